"""Hostile frames and probes for the grid-window searches, and an independent definition of the family.

Plain numpy: nothing here touches the device or the oracle.  The definition is written from the reference
(src/cMultiFrame.cpp:272-353, src/cORBmatcher.cpp:67-175, 326-726, 1990-2118): the 64x48 grid built literally, GetFeaturesInArea
with its four early returns, and the sequential loops of the rules.  Every double -> int conversion goes through x86_int(), the result
the reference has as built on x86-64: INT_MIN for NaN and for anything outside int range.

A case is a dict: name, group, rule, frame, probes, nnratio, th, max_dist, dim, plus what its non-vacuity check needs.
  rule   0 SearchByProjection(F, mapPoints, th)   1 WindowSearch   2 SearchByProjection(Cur, Last)   3 SearchForInitialization
         "best" independent best-in-window   "best_taken" best-in-window that skips and takes features (max_dist replaces TH_HIGH)
  frame  keys (KP_DTYPE), desc / mask [n, stride] (mask None: no masks), cam, width, height, scales, assigned
  probes x, y, cam, desc, mask and  r, lo, hi  (rule 0: view_cos, level  instead)
run(case) -> match, nmatches, assigned, accepted, dist, trace.
"""
import numpy as np

INT_MIN, INT_MAX = -2**31, 2**31 - 1
COLS, ROWS = 64, 48          # FRAME_GRID_COLS / ROWS
LIST_K = 16                  # length of the device's short lists (kProjListK); only the non-vacuity trace uses it
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
SCALES = np.array([1.2 ** k for k in range(8)], np.float64)
NAN, INF = float("nan"), float("inf")


def x86_int(v):
    """cvttsd2si / cvtsd2si of an already integral double: INT_MIN ("integer indefinite") unless -2^31 - 1 < v < 2^31.  Arrays or scalars."""
    v = np.asarray(v, np.float64)
    ok = (v > -2147483649.0) & (v < 2147483648.0)          # NaN fails both
    return np.where(ok, np.where(ok, v, 0.0), float(INT_MIN)).astype(np.int64)


def cv_round(v):
    return x86_int(np.rint(v))                              # round-half-even, then the conversion


def thresholds(dim, masks):                                 # TH_HIGH_, TH_LOW_ (src/cORBmatcher.cpp:46-65)
    return (int(np.floor(1.5 * dim)), int(np.floor(float(dim)))) if masks else (3 * dim, 2 * dim)


class Grid:
    """mGrids of one frame: per camera 64 x 48 lists of feature indices in mvKeys order"""

    def __init__(self, F):
        nr = len(F["width"])
        self.wInv = [float(COLS) / float(int(w) - 0) for w in F["width"]]
        self.hInv = [float(ROWS) / float(int(h) - 0) for h in F["height"]]
        self.cells = [[[[] for _ in range(ROWS)] for _ in range(COLS)] for _ in range(nr)]
        keys, cam = F["keys"], F["cam"]
        self.kx, self.ky = keys["x"].astype(np.float64).tolist(), keys["y"].astype(np.float64).tolist()
        self.oct = keys["octave"].tolist()
        self.cell_of = np.full(len(keys), -1, np.int64)
        if len(keys):
            wi, hi = np.array(self.wInv)[cam], np.array(self.hInv)[cam]
            px = cv_round((keys["x"].astype(np.float64) - 0) * wi)      # PosInGrid
            py = cv_round((keys["y"].astype(np.float64) - 0) * hi)
            for i in range(len(keys)):
                gx, gy = int(px[i]), int(py[i])
                if gx < 0 or gx >= COLS or gy < 0 or gy >= ROWS:
                    continue
                self.cells[int(cam[i])][gx][gy].append(i)
                self.cell_of[i] = gx * ROWS + gy

    def features_in_area(self, cam, x, y, r, lo=-1, hi=-1):
        out = []
        w, h = self.wInv[cam], self.hInv[cam]
        x0 = max(0, int(x86_int(np.floor((x - 0 - r) * w))))
        if x0 >= COLS:
            return out
        x1 = min(COLS - 1, int(x86_int(np.ceil((x - 0 + r) * w))))
        if x1 < 0:
            return out
        y0 = max(0, int(x86_int(np.floor((y - 0 - r) * h))))
        if y0 >= ROWS:
            return out
        y1 = min(ROWS - 1, int(x86_int(np.ceil((y - 0 + r) * h))))
        if y1 < 0:
            return out
        check, same = True, False
        if lo == -1 and hi == -1:
            check = False
        elif lo == hi:
            same = True
        kx, ky, octv, cells = self.kx, self.ky, self.oct, self.cells[cam]
        for ix in range(x0, x1 + 1):
            col = cells[ix]
            for iy in range(y0, y1 + 1):
                for j in col[iy]:
                    if check and not same:
                        if octv[j] < lo or octv[j] > hi:
                            continue
                    elif same:
                        if octv[j] != lo:
                            continue
                    if abs(kx[j] - x) > r or abs(ky[j] - y) > r:
                        continue
                    out.append(j)
        return out


def distances(P, row, F, idx, dim):
    """descriptor distance of probe row `row` to the frame rows idx; masked: (|x & m1| + |x & m2|) / 2, halved once"""
    idx = np.asarray(idx, np.int64)
    x = P["desc"][row, :dim][None, :] ^ F["desc"][idx, :dim]
    if P["mask"] is None:
        return np.unpackbits(x, axis=1).sum(axis=1).astype(np.int64)
    a = np.unpackbits(x & P["mask"][row, :dim][None, :], axis=1).sum(axis=1).astype(np.int64)
    b = np.unpackbits(x & F["mask"][idx, :dim], axis=1).sum(axis=1).astype(np.int64)
    return (a + b) >> 1


def probe_window(case, p):
    """(radius, min level, max level) of probe p"""
    P, F = case["probes"], case["frame"]
    if case["rule"] == 0:
        lvl = int(P["level"][p])
        r = 2.5 if float(P["view_cos"][p]) > 0.998 else 4.0          # RadiusByViewingCos
        if case["th"] != 1.0:
            r *= case["th"]
        return r * float(F["scales"][lvl]), lvl - 1, lvl
    return float(P["r"][p]), int(P["lo"][p]), int(P["hi"][p])


def run(case, skip=(), grid=None, only=None):
    """The sequential definition.  skip: probes left out (they end unmatched); only: stop after this probe."""
    F, P, rule, dim = case["frame"], case["probes"], case["rule"], case["dim"]
    masks = P["mask"] is not None
    TH_HIGH, TH_LOW = thresholds(dim, masks)
    if rule in ("best", "best_taken"):
        TH_HIGH = case["max_dist"]
    ratio = case["nnratio"]
    G = grid or Grid(F)
    n, nf = len(P["cam"]), len(F["keys"])
    match, accepted, dist_out = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, INT_MAX, np.int32)
    assigned = F["assigned"].copy()
    mdist, owner = [INT_MAX] * nf, [-1] * nf
    nmatches = steals = 0
    trace = [None] * n
    octv = G.oct
    for p in range(n):
        if p in skip:
            continue
        if only is not None and p > only:
            break
        r, lo, hi = probe_window(case, p)
        members = G.features_in_area(int(P["cam"][p]), float(P["x"][p]), float(P["y"][p]), r, lo, hi)
        if not members:
            trace[p] = dict(members=0)
            continue
        d = distances(P, p, F, members, dim).tolist()
        best = best2 = INT_MAX
        lvl1 = lvl2 = -1
        bi = si = -1
        free = []
        for k, i in enumerate(members):
            dist = d[k]
            if rule == 3:
                ok = not (mdist[i] <= dist)
            elif rule == "best":
                ok = True
            else:
                ok = not assigned[i]
            free.append(ok)
            if not ok:
                continue
            if dist < best:
                best2, lvl2, si = best, lvl1, bi
                best, lvl1, bi = dist, octv[i], i
            elif dist < best2:
                best2, lvl2, si = dist, octv[i], i
        # what the device's short list would hold at this probe's turn (non-vacuity only)
        order = sorted(range(len(members)), key=lambda k: (d[k], k))[:LIST_K]
        nfree = sum(free[k] for k in order)
        full = len(members) > LIST_K
        dK = d[order[-1]] if full else INT_MAX
        th_rule = TH_LOW if rule == 3 else TH_HIGH
        sit = None
        if full and rule != "best":
            if nfree == 0:
                sit = "C" if dK <= th_rule else "D"
            elif nfree == 1 and rule != 2 and rule != "best_taken" and best <= th_rule:
                if rule == 0:
                    passes = not (float(best) > ratio * float(dK))
                elif rule == 1:
                    passes = float(best) <= float(dK) * ratio
                else:
                    passes = float(best) < float(dK) * ratio
                sit = "A" if passes else "B"
        trace[p] = dict(members=len(members), listed_free=nfree, full=full, situation=sit, best=bi, second=si, best_dist=best, second_dist=best2,
                        best_cell=int(G.cell_of[bi]) if bi >= 0 else -1, lowest_tied=min([i for k, i in enumerate(members) if free[k] and d[k] == best], default=-1))
        if rule == 0:                                   # :153-163
            if best <= TH_HIGH:
                if lvl1 == lvl2 and float(best) > ratio * float(best2):
                    continue
                assigned[bi] = 1
                match[p] = bi
                nmatches += 1
        elif rule == 1:                                 # :416
            if float(best) <= float(best2) * ratio and best <= TH_HIGH:
                assigned[bi] = 1
                match[p] = bi
                nmatches += 1
        elif rule in (2, "best_taken"):                 # :2072 / :2120-2263
            if bi >= 0 and best <= TH_HIGH:
                assigned[bi] = 1
                match[p] = bi
                nmatches += 1
                if rule == "best_taken":
                    dist_out[p] = best
        elif rule == 3:                                 # :662-681
            if best <= TH_LOW:
                if float(best) < float(best2) * ratio:
                    if owner[bi] >= 0:
                        match[owner[bi]] = -1
                        nmatches -= 1
                        steals += 1
                    match[p] = bi
                    owner[bi] = p
                    mdist[bi] = best
                    nmatches += 1
                    accepted[p] = bi
        else:                                           # independent best
            if bi < 0:
                continue
            dist_out[p] = best
            if best <= TH_HIGH:
                match[p] = bi
                nmatches += 1
    return dict(match=match, nmatches=nmatches, assigned=assigned, accepted=accepted, dist=dist_out, trace=trace, steals=steals)


# ---------------------------------------------------------------------------------------------- builders
def keys_of(xy, octave=0):
    k = np.zeros(len(xy), KP_DTYPE)
    if len(xy):
        xy = np.asarray(xy, np.float64)
        k["x"], k["y"] = xy[:, 0].astype(np.float32), xy[:, 1].astype(np.float32)
    k["octave"] = octave
    k["size"] = 31.0
    return k


def padded(rows, stride, rng):
    """rows [n, dim] inside rows of `stride` bytes; the padding holds random bytes"""
    rows = np.ascontiguousarray(rows, np.uint8)
    if stride == rows.shape[1]:
        return rows
    out = rng.integers(0, 256, (rows.shape[0], stride), dtype=np.uint8)
    out[:, :rows.shape[1]] = rows
    return out


def frame(keys, desc, cam=None, size=(128, 96), nr_cams=1, mask=None, assigned=None):
    n = len(keys)
    w, h = size
    return dict(keys=keys, desc=np.ascontiguousarray(desc, np.uint8), mask=None if mask is None else np.ascontiguousarray(mask, np.uint8),
                cam=np.zeros(n, np.int32) if cam is None else np.asarray(cam, np.int32),
                width=np.full(nr_cams, w, np.int32), height=np.full(nr_cams, h, np.int32), scales=SCALES.copy(),
                assigned=np.zeros(n, np.uint8) if assigned is None else np.asarray(assigned, np.uint8))


def probes(x, y, r, desc, lo=-1, hi=-1, cam=0, mask=None):
    n = len(x)
    full = lambda v, t: np.full(n, v, t) if np.isscalar(v) else np.ascontiguousarray(v, t)
    return dict(x=np.ascontiguousarray(x, np.float64), y=np.ascontiguousarray(y, np.float64), r=full(r, np.float64), lo=full(lo, np.int32), hi=full(hi, np.int32),
                cam=full(cam, np.int32), desc=np.ascontiguousarray(desc, np.uint8), mask=None if mask is None else np.ascontiguousarray(mask, np.uint8))


def probes0(x, y, view_cos, level, desc, cam=0, mask=None):
    n = len(x)
    full = lambda v, t: np.full(n, v, t) if np.isscalar(v) else np.ascontiguousarray(v, t)
    return dict(x=np.ascontiguousarray(x, np.float64), y=np.ascontiguousarray(y, np.float64), view_cos=full(view_cos, np.float64), level=full(level, np.int32),
                cam=full(cam, np.int32), desc=np.ascontiguousarray(desc, np.uint8), mask=None if mask is None else np.ascontiguousarray(mask, np.uint8))


def case(name, group, rule, F, P, nnratio=0.8, th=1.0, max_dist=None, dim=32, **extra):
    c = dict(name=name, group=group, rule=rule, frame=F, probes=P, nnratio=nnratio, th=th, dim=dim,
             max_dist=thresholds(dim, P["mask"] is not None)[0] if max_dist is None else max_dist)
    c.update(extra)
    return c


def weight_rows(weights, dim=32, offset=0):
    """descriptor rows whose first `w` bits (from bit `offset` on) are set: distance w from the all-zero row"""
    out = np.zeros((len(weights), dim * 8), np.uint8)
    for i, w in enumerate(weights):
        out[i, offset:offset + int(w)] = 1
    return np.packbits(out, axis=1)


def as_rule0(c, name, th, level=0, view_cos=0.5):
    """the same frame and centres under rule 0: radius (2.5 | 4) * th * scales[level], levels [level - 1, level]"""
    P = c["probes"]
    return case(name, c["group"], 0, c["frame"], probes0(P["x"], P["y"], view_cos, level, P["desc"], P["cam"], P["mask"]), c["nnratio"], th, None, c["dim"],
                **{k: v for k, v in c.items() if k in ("links", "tie", "cluster", "collide")})


def with_rule(c, rule, name=None, **kw):
    d = dict(c)
    d.update(rule=rule, name=name or "%s/r%s" % (c["name"], rule))
    d.update(kw)
    return d


def levels(P, lo, hi):
    """the same probes with another level range"""
    n = len(P["cam"])
    return dict(P, lo=np.full(n, lo, np.int32), hi=np.full(n, hi, np.int32))


def twice(P):
    """the probe list repeated: under a taking rule the second pass shows each window's next member"""
    return {k: (None if v is None else np.concatenate([v, v])) for k, v in P.items()}


# ---------------------------------------------------------------------------------------------- geometry
PINNED_FEATURES = [(1, 1), (3, 3), (5, 5), (60, 40), (126.9, 50), (127, 50)]
PINNED = [  # probe (x, y, r) -> window_best's answer on x86 (the issue's list; -1 = no match)
    ((NAN, 1, 5), -1), ((1, NAN, 5), -1), ((1, 1, INF), -1), ((1, 1, 1e300), -1), ((1, 1, NAN), -1), ((60, 40, 1e10), -1),
    ((1e300, 1, 5), -1), ((-1e300, 1, 5), -1), ((60, 40, 3e9), 0), ((127, 50, 0.5), 4),
]


def pinned_case():
    F = frame(keys_of(PINNED_FEATURES), np.zeros((6, 32), np.uint8))
    xyr = np.array([p for p, _ in PINNED], np.float64)
    return case("pinned", "geometry", "best", F, probes(xyr[:, 0], xyr[:, 1], xyr[:, 2], np.zeros((len(xyr), 32), np.uint8)),
                expect=np.array([m for _, m in PINNED], np.int32))


def lattice_frame(size, rng, nonfinite=False):
    """keypoints whose bins are exactly k + 0.5 where the grid factor allows (128 x 96: odd x and y), on every octave; bins 64 / 48 included"""
    w, h = size
    fx, fy = w / 64.0, h / 48.0
    xs = [(k + 0.5) * fx for k in list(range(0, 64, 3)) + [62, 63]]          # the last bins to 64 at w = 128 (63.5 -> 64) and is dropped
    ys = [(k + 0.5) * fy for k in (0, 1, 2, 20, 21, 45, 46, 47)]
    xy = [(x, y) for x in xs for y in ys]
    xy += [(w - 0.01, 10.0), (w - 0.6 * fx, 10.0), (10.0, h - 0.01), (10.0, h - 0.6 * fy), (0.0, 0.0), (-0.4 * fx, 5.0), (-0.6 * fx, 5.0), (5.0, -0.6 * fy)]
    keys = keys_of(xy)
    keys["octave"] = np.arange(len(keys)) % 8
    if nonfinite:
        bad = keys_of([(1, 1)] * 10)
        bad["x"][:6] = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9]
        bad["y"][6:] = [np.nan, np.inf, 2.0 ** 33, -3e9]
        bad["x"][9], bad["y"][0] = np.nan, 1.0
        keys = np.concatenate([bad, keys])
    return frame(keys, rng.integers(0, 256, (len(keys), 32), dtype=np.uint8), size=size)


def geometry_probes(size, rng):
    w, h = size
    fx, fy = w / 64.0, h / 48.0
    x1, y1 = 3.5 * fx, 0.5 * fy                    # a lattice keypoint
    xyr = [
        (x1 - 0.75, y1, 0.75), (x1 - 0.75, y1, np.nextafter(0.75, 0.0)), (x1, y1 + 0.75, 0.75), (x1, y1 + 0.75, np.nextafter(0.75, 0.0)),   # |kp - x| == r; just above r
        (x1, y1, 0.0), (x1, y1, -1.0), (x1, y1, -0.0), (x1, y1, fx / 2), (x1 + fx / 2, y1, fx / 2), (w / 2, h / 2, fx / 2),              # r = 0, r < 0, half a cell
        (-50.0, h / 2, 5.0), (w + 80.0, h / 2, 5.0), (w / 2, -50.0, 5.0), (w / 2, h + 80.0, 5.0),                                          # the four early returns, each alone
        (-3.0, 0.5 * fy, 3.0 + 0.5 * fx), (w + 3.0, 10.0, 3.0 + fx), (5.0, -3.0, 3.0 + 0.5 * fy), (10.0, h + 3.0, 3.0 + fy), (-30.0, -30.0, 60.0),  # centred outside, reaching in
        (w + 30.0, h + 30.0, 70.0), (w / 2, h / 2, 1e4), (w / 2, h / 2, 3e9), (w / 2, h / 2, 1e10), (0.0, 0.0, 2.0 ** 31 * fx),
        (NAN, 1, 5), (1, NAN, 5), (1, 1, INF), (1, 1, -INF), (1, 1, 1e300), (1, 1, NAN), (INF, 1, 5), (-INF, 1, 5), (1, INF, 5), (1e300, 1, 5), (-1e300, 1, 5),
        (1, 1e300, 5), (INF, INF, INF), (3e9, 1, 3e9), (-3e9, 1, 3.1e9), (1, 1, 5), (w - 1.0, 10.0, 3.0), (10.0, h - 1.0, 3.0),
    ]
    for _ in range(24):
        xyr.append((rng.uniform(-10, w + 10), rng.uniform(-10, h + 10), rng.choice([0.5, 1.0, 2.0, 3.5, 7.0, 30.0]) * fx))
    return np.array(xyr, np.float64)


LEVEL_MODES = [(-1, -1), (3, 3), (0, 0), (7, 7), (2, 5), (0, 7), (5, 2), (-1, 3), (0, INT_MAX), (-1, 0), (6, 7), (-2, -2), (INT_MIN, INT_MAX)]


def geometry_cases(rng):
    out = [pinned_case()]
    for size in ((128, 96), (754, 480)):
        for nonfinite in (False, True):
            F = lattice_frame(size, rng, nonfinite)
            xyr = geometry_probes(size, rng)
            tag = "%dx%d%s" % (size[0], size[1], "/nonfinite-keys" if nonfinite else "")
            P = probes(xyr[:, 0], xyr[:, 1], xyr[:, 2], rng.integers(0, 256, (len(xyr), 32), dtype=np.uint8))
            out.append(case("geometry/" + tag + "/best", "geometry", "best", F, P, max_dist=256))
            out.append(case("geometry/" + tag + "/taken", "geometry", "best_taken", F, twice(P), max_dist=256))
            if not nonfinite:
                out.append(case("geometry/" + tag + "/r1", "geometry", 1, F, twice(P), nnratio=1.0))
                out.append(case("geometry/" + tag + "/r3", "geometry", 3, F, twice(probes(xyr[:, 0], xyr[:, 1], xyr[:, 2], P["desc"], 0, 0)), nnratio=1.0))
            # rule 0: any radius comes through th; levels [lvl - 1, lvl] at level 0 and at the top level
            P0 = probes0(xyr[:, 0], xyr[:, 1], np.where(np.arange(len(xyr)) % 2 == 0, 0.5, 0.9999), np.arange(len(xyr)) % 8, P["desc"])
            for th in (1.0, 0.0, -1.0, 7.5, INF, NAN, 1e300):
                out.append(case("geometry/%s/r0/th=%r" % (tag, th), "geometry", 0, F, twice(P0), th=th))
        # level modes on keypoints of every octave: one wide window per mode
        F = lattice_frame(size, rng)
        lo, hi = np.array(LEVEL_MODES, np.int64).T
        m = len(LEVEL_MODES)
        P = probes(np.full(m, size[0] / 2.0), np.full(m, size[1] / 2.0), float(size[0]), np.zeros((m, 32), np.uint8), lo, hi)
        P = {k: (None if v is None else np.repeat(v, 9, axis=0)) for k, v in P.items()}     # nine takes per mode: one more than the octaves
        out.append(case("levels/%dx%d/taken" % size, "geometry", "best_taken", F, P, max_dist=256))
        out.append(case("levels/%dx%d/best" % size, "geometry", "best", F, P, max_dist=256))
        P0 = probes0(np.full(16, size[0] / 2.0), np.full(16, size[1] / 2.0), 0.5, np.repeat([0, 7], 8), np.zeros((16, 32), np.uint8))
        out.append(case("levels/%dx%d/r0" % size, "geometry", 0, F, P0, th=1000.0, nnratio=1.0))
    # two to five cameras with features at identical pixel positions: only the probe's camera counts
    for nr in (2, 3, 5):
        xy = rng.uniform(5, 120, (30, 2))
        keys = keys_of(np.tile(xy, (nr, 1)))
        cam = rng.permutation(np.repeat(np.arange(nr), 30)).astype(np.int32)
        F = frame(keys, rng.integers(0, 256, (len(keys), 32), dtype=np.uint8), cam=cam, nr_cams=nr)
        F["width"][:], F["height"][:] = 128 + 10 * np.arange(nr), 96 + 6 * np.arange(nr)      # the cameras differ in size too
        pc = rng.integers(0, nr, 40).astype(np.int32)
        pxy = xy[rng.integers(0, 30, 40)]
        P = probes(pxy[:, 0], pxy[:, 1], 12.0, rng.integers(0, 256, (40, 32), dtype=np.uint8), cam=pc)
        out.append(case("cameras/%d/best" % nr, "geometry", "best", F, P, max_dist=256))
        out.append(case("cameras/%d/r1" % nr, "geometry", 1, F, P, nnratio=0.95))
    return out


# ---------------------------------------------------------------------------------------------- decisions
def decision_cases(rng):
    out = []
    for dim in (16, 32, 64):
        for masked in (False, True):
            TH_HIGH, TH_LOW = thresholds(dim, masked)
            # one feature per probe, 8 px apart; distances TH, TH + 1 for every threshold a rule reads
            dists = [TH_HIGH, TH_HIGH + 1, TH_LOW, TH_LOW + 1, 0, 1, TH_HIGH - 1, TH_LOW - 1]
            n = len(dists)
            xy = np.stack([10.0 + 12.0 * np.arange(n), np.full(n, 20.0)], axis=1)
            fd = rng.integers(0, 256, (n, dim), dtype=np.uint8)
            pd = fd.copy()
            fm = pm = None
            if masked:
                # masks all-ones on the frame side; the probe's mask drops one differing bit, so the sum is odd before halving where wanted:
                # x differing bits, m of them under the probe's mask -> (m + x) >> 1.  Choose m = x (even sum) or m = x - 1 with one more flip (odd sum).
                fm, pm = np.full((n, dim), 255, np.uint8), np.full((n, dim), 255, np.uint8)
            bits = np.unpackbits(pd, axis=1)
            for i, d in enumerate(dists):
                flip = rng.permutation(dim * 8)[:d + 1]
                bits[i, flip[:d]] ^= 1
                if masked and i % 2 == 0:                       # one more differing bit, hidden from the probe's mask: (d + d + 1) >> 1 == d, odd before halving
                    bits[i, flip[d]] ^= 1
                    mb = np.unpackbits(pm[i])
                    mb[flip[d]] = 0
                    pm[i] = np.packbits(mb)
            pd = np.packbits(bits, axis=1)
            for stride in (dim, dim + 12):
                F = frame(keys_of(xy), padded(fd, stride, rng), size=(754, 480), mask=None if fm is None else padded(fm, stride, rng))
                ps = stride if stride == dim else dim + 4
                P = probes(xy[:, 0], xy[:, 1], 3.0, padded(pd, ps, rng), 0, 0, mask=None if pm is None else padded(pm, ps, rng))
                tag = "decision/dim%d%s%s" % (dim, "/masked" if masked else "", "/strided" if stride != dim else "")
                for rule in (1, 2, 3, "best"):
                    out.append(case("%s/r%s" % (tag, rule), "decision", rule, F, P, dim=dim))
                out.append(as_rule0(out[-1], tag + "/r0", th=0.75))
                for md in (0, TH_LOW, TH_LOW + 1, 3 * dim + 1):
                    out.append(case("%s/best/max%d" % (tag, md), "decision", "best", F, P, dim=dim, max_dist=md))
                    out.append(case("%s/taken/max%d" % (tag, md), "decision", "best_taken", F, P, dim=dim, max_dist=md))
    # four windows of radius 2.5 (weights = distances from the all-zero probes; octaves 0 0 | 1 0 | 0 | 0 0 1):
    #   (20..22)    10 and 20 at nnratio 0.5: the exact ratio tie.  Rules 0 and 1 accept (<=), rule 3 rejects (strict <)
    #   (60..62)    30 on octave 1, 25 on octave 0            (100) a single member: second = INT_MAX
    #   (140..144)  10, 21 on octave 0 and 19 on octave 1: the runner-up is closer but on another octave, so rule 0 applies no ratio (10 > 0.5 * 19)
    keys = keys_of([(20, 20), (22, 20), (60, 20), (62, 20), (100, 20), (140, 20), (142, 20), (144, 20)])
    keys["octave"] = [0, 0, 1, 0, 0, 0, 0, 1]
    fd = weight_rows([10, 20, 30, 25, 7, 10, 21, 19])
    F = frame(keys, fd, size=(754, 480))
    P = probes([21, 61, 100, 142], [20, 20, 20, 20], 2.5, np.zeros((4, 32), np.uint8), 0, 0)
    for rule in (1, 3):
        out.append(case("decision/ratio-tie/r%d" % rule, "decision", rule, F, P, nnratio=0.5))
    P1 = probes([21, 61, 100, 142], [20, 20, 20, 20], 2.5, np.zeros((4, 32), np.uint8))      # no level check: the octave-1 features are members
    out.append(case("decision/ratio-tie/r1-all-levels", "decision", 1, F, P1, nnratio=0.5))
    # rule 0 at level 1 has levels [0, 1], so every feature is a member; at level 0 the octave-1 features drop out
    # window (140..144): best 10 (octave 0), runner-up 19 on octave 1 (closer than the 21 on octave 0): the ratio is not applied although 10 > 0.5 * 19
    out.append(case("decision/ratio-tie/r0", "decision", 0, F, probes0(P["x"], P["y"], 0.5, 1, P["desc"]), nnratio=0.5, th=2.5 / 4.0 / 1.2))
    out.append(case("decision/ratio-tie/r0-level0", "decision", 0, F, probes0(P["x"], P["y"], 0.5, 0, P["desc"]), nnratio=0.5, th=2.5 / 4.0))
    return out


# ---------------------------------------------------------------------------------------------- visiting order
def order_cases(rng):
    """equal distances: the first member in GetFeaturesInArea order wins (column-major cells, then the index), not the lowest index"""
    # 754 x 480: cells are 11.78 x 10 px.  Features listed so that higher indices lie in EARLIER columns / rows.
    xy = [(200, 100), (150, 100), (100, 100),            # one row, three columns: index 2 is visited first
          (300, 250), (300, 230), (300, 210),            # one column, three rows: index 5 first
          (400, 300), (401, 300), (400.5, 300.5),        # one cell: the index decides
          (500, 100), (480, 130), (520, 70), (480, 70)]  # a later column with a lower index against an earlier column, both rows
    n = len(xy)
    out = []
    one = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    for name, fd, pd in (("zero", np.zeros((n, 32), np.uint8), np.zeros((4, 32), np.uint8)),
                         ("equal", np.tile(one, (n, 1)), np.tile(one, (4, 1)) ^ weight_rows([3, 5, 7, 9]))):
        F = frame(keys_of(xy), fd, size=(754, 480))
        P = probes([150, 300, 400, 500], [100, 230, 300, 100], 60.0, pd)
        for rule in ("best", 1, 2, 3)[:3 if name == "zero" else 4]:      # rule 3 compares with strict '<': equal distances of 0 never match
            c = case("order/%s/r%s" % (name, rule), "order", rule, F, twice(twice(P)) if rule != "best" else P, nnratio=1.0, max_dist=256, tie=True)
            if rule == 3:
                c["probes"]["lo"][:] = 0
                c["probes"]["hi"][:] = 0
                c["nnratio"] = 1.5          # strict '<' against an equal runner-up passes only above 1
            out.append(c)
        out.append(as_rule0(out[-1], "order/%s/r0" % name, th=15.0))
        out[-1]["nnratio"] = 1.0
    return out


# ---------------------------------------------------------------------------------------------- clusters
def cluster_frame(m, rng, near=True, size=(754, 480)):
    """m features inside one 6 x 6 px patch around (300, 200) (two columns, two rows of cells), descriptors base + 8 flipped bits each (near: pairwise
    distance 16, 8 from the base) or independent random rows (far)"""
    xy = np.stack([297.0 + rng.integers(0, 7, m), 197.0 + rng.integers(0, 7, m)], axis=1)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    if near:
        bits = np.tile(np.unpackbits(base), (m, 1))
        for i in range(m):
            bits[i, rng.permutation(256)[:8]] ^= 1
        fd = np.packbits(bits, axis=1)
    else:
        fd = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    return frame(keys_of(xy), fd, size=size), base


def cluster_cases(rng):
    out = []
    for m in (16, 17, 40, 200):
        # identical descriptors: every probe's list is the first 16 members in visiting order
        F, base = cluster_frame(m, rng)
        F["desc"][:] = base
        nprobe = 48
        pd = np.tile(base, (nprobe, 1))
        pd[40:] ^= 255                                              # the last eight are 256 away: dK > TH with every listed key taken
        P = probes(np.full(nprobe, 300.0), np.full(nprobe, 200.0), 8.0, pd, 0, 0)
        for rule in (1, 2, 0):
            c = case("cluster/identical/%d/r%s" % (m, rule), "cluster", rule, F, levels(P, -1, -1), nnratio=0.8, cluster=m)
            out.append(c if rule else as_rule0(c, c["name"], th=2.0))
        # near-identical descriptors and a frame part of which is assigned on entry
        F, base = cluster_frame(m, rng)
        asg = (rng.random(m) < 0.5).astype(np.uint8)
        F["assigned"] = asg
        pd = F["desc"][rng.integers(0, m, nprobe)].copy()
        pd[::3] = base
        P = probes(np.full(nprobe, 300.0), np.full(nprobe, 200.0), 8.0, pd, 0, 0)
        for rule in (1, 2, 0, 3):
            for ratio in (0.8, 1.0):
                c = case("cluster/near/%d/r%s/ratio%.1f" % (m, rule, ratio), "cluster", rule, F, P, nnratio=ratio, cluster=m)
                out.append(c if rule else as_rule0(c, c["name"], th=2.0))
        Fall = dict(F)
        Fall["assigned"] = np.ones(m, np.uint8)                     # a window in which every member is assigned
        for rule in (1, 2):
            out.append(case("cluster/all-assigned/%d/r%s" % (m, rule), "cluster", rule, Fall, P, cluster=m))
        out.append(as_rule0(out[-1], "cluster/all-assigned/%d/r0" % m, th=2.0))
    out += situation_cases(rng)
    return out


def situation_cases(rng):
    """the four situations of a probe whose short list is (almost) used up, built by hand for every rule that has them.
    One cluster of 40: weights (distance from the all-zero probe) in visiting order.  A first wave of probes, or `assigned`, uses up the list."""
    out = []
    m = 40
    xy = np.stack([297.0 + (np.arange(m) % 7), 197.0 + (np.arange(m) // 7)], axis=1)

    def fr(weights, assigned=None):
        return frame(keys_of(xy), weight_rows(weights), size=(754, 480), assigned=assigned)

    def zero_probes(n):
        return probes(np.full(n, 300.0), np.full(n, 200.0), 8.0, np.zeros((n, 32), np.uint8), 0, 0)

    for rule in (0, 1):
        def emit(name, F, P, **kw):
            c = case("situation/%s/r%d" % (name, rule), "cluster", rule, F, P, cluster=m, **kw)
            out.append(c if rule else as_rule0(c, c["name"], th=2.0))
        # A: fourteen listed keys at 0 assigned, one free at 2, the sixteenth at 10 assigned; hidden ones at 10 and more -> accepted against the bound
        w = np.array([0] * 14 + [2, 10] + [10] * 10 + [30] * 14)
        a = np.zeros(m, np.uint8); a[:14] = 1; a[15] = 1
        emit("A", fr(w, a), zero_probes(1), nnratio=0.8)
        # B: the one free listed key IS the sixteenth (5 = dK), hidden runner-up at 10: only the rescan shows 5 <= 0.8 * 10
        w = np.array([0] * 15 + [5] + [10] * 24)
        a = np.zeros(m, np.uint8); a[:15] = 1
        emit("B-accept", fr(w, a), zero_probes(1), nnratio=0.8)
        # B: the same with the hidden runner-up at 6: rejected, and only after the rescan
        w = np.array([0] * 15 + [5] + [6] * 24)
        emit("B-reject", fr(w, a), zero_probes(1), nnratio=0.8)
        # C: all sixteen assigned, dK <= TH: the rescan finds the free hidden members
        w = np.array([0] * 16 + [7, 20] + [40] * 22)
        a = np.zeros(m, np.uint8); a[:16] = 1
        emit("C", fr(w, a), zero_probes(3), nnratio=0.8)
        # D: all sixteen assigned and dK > TH: no match without a rescan
        w = np.array([97] * 16 + [100] * 24)
        emit("D", fr(w, a), zero_probes(2), nnratio=0.8)
        # forty probes on one cluster: the first sixteen use the list up, the rest meet C; the weights rise slowly enough for the ratio
        w = np.array([0] * 30 + [40] * 10)
        emit("forty", fr(w), zero_probes(44), nnratio=0.8)
    # rule 3: a key is "taken" for a probe once it is matched at a distance <= the probe's.  Wave 1 matches every feature but two at distance 0.
    F, base = cluster_frame(m, rng)
    F["keys"] = keys_of(xy)
    free = (3, 9)
    wave1 = [i for i in range(m) if i not in free]
    pd = np.concatenate([F["desc"][wave1], F["desc"][[free[0]]], np.tile(base, (14, 1)), F["desc"][wave1[:12]]])
    out.append(case("situation/steal-waves/r3", "cluster", 3, F, probes(np.full(len(pd), 300.0), np.full(len(pd), 200.0), 8.0, pd, 0, 0), nnratio=0.9, cluster=m))
    Ff, _ = cluster_frame(m, rng, near=False)
    Ff["keys"] = keys_of(xy)
    pd = np.concatenate([Ff["desc"], Ff["desc"][:14]])
    out.append(case("situation/far/r3", "cluster", 3, Ff, probes(np.full(len(pd), 300.0), np.full(len(pd), 200.0), 8.0, pd, 0, 0), nnratio=0.9, cluster=m))
    return out


# ---------------------------------------------------------------------------------------------- chains
def chain_cases():
    """150 probes; probe j sees features j - 1 and j exactly (|kp - x| == r on both sides).  Its best is feature j at 10, its runner-up feature j - 1 at 12:
    rejected by the ratio (10 > 0.8 * 12) unless probe j - 1 took feature j - 1 first, which it does if probe j - 2 ... down to probe 0, which sees one
    feature.  Every link crosses into the next probe; links 63/64 and 127/128 cross the device's 64-probe rounds."""
    n = 150
    xy = np.stack([10.0 + 4.0 * np.arange(n), np.full(n, 20.0)], axis=1)
    fbits = np.zeros((n, 256), np.uint8)
    pbits = np.zeros((n, 256), np.uint8)
    for j in range(n):
        fbits[j, j % 3] = 1
        pbits[j, j % 3] = 1
        pbits[j, 8:18] = 1
    F = frame(keys_of(xy), np.packbits(fbits, axis=1), size=(754, 480))
    P = probes(xy[:, 0] - 2.0, xy[:, 1], 2.0, np.packbits(pbits, axis=1), 0, 0)
    links = list(range(1, n))
    out = [case("chain/r1", "chain", 1, F, levels(P, -1, -1), nnratio=0.8, links=links), case("chain/r3", "chain", 3, F, P, nnratio=0.8, links=links)]
    out.append(as_rule0(out[0], "chain/r0", th=0.5))
    return out


# ---------------------------------------------------------------------------------------------- claim-table collisions
def collision_cases(rng):
    """4200 features: features i and i + 4096 (i < 104) share a slot of the device's 4096-entry claim table.  Probe 2i looks at feature i alone, probe 2i + 1
    at feature i + 4096 and its neighbour i + 4097 - or, for the last, feature 103 + 1: both probes fall in one 64-probe round, and the claim of the first
    sits in the slot that the best and, for every other pair, the runner-up of the second hash to."""
    nf, k = 4200, 104
    xy = rng.uniform(0, 750, (nf, 2))
    cam = np.ones(nf, np.int32)
    loc = np.stack([20.0 + 7.0 * (np.arange(k) % 100), 30.0 + 200.0 * (np.arange(k) // 100)], axis=1)
    xy[:k] = loc
    xy[4096:] = loc + [0.0, 100.0]
    cam[:k] = 0
    cam[4096:] = 0
    fd = rng.integers(0, 256, (nf, 32), dtype=np.uint8)
    fd[:k] = weight_rows([12] * k)
    fd[4096:] = weight_rows([10, 14] * (k // 2), offset=100)
    F = frame(keys_of(xy), fd, cam=cam, size=(754, 480), nr_cams=2)
    # even pairs: radius 1 around feature i + 4096 alone; odd pairs: the window also holds feature i + 4095 (7 px to the left), whose slot pair 2i - 2 claimed
    px = np.stack([loc[:, 0], loc[:, 0] - 3.5 * (np.arange(k) % 2)], axis=1).reshape(-1)
    py = np.stack([loc[:, 1], loc[:, 1] + 100.0], axis=1).reshape(-1)
    P = probes(px, py, 4.0, np.zeros((2 * k, 32), np.uint8))
    out = [case("collision/r1", "collision", 1, F, P, nnratio=0.8, collide=True), case("collision/r3", "collision", 3, F, levels(P, 0, 0), nnratio=0.8, collide=True),
           case("collision/r2", "collision", 2, F, P, collide=True)]
    out.append(as_rule0(out[0], "collision/r0", th=1.0))
    return out


# ---------------------------------------------------------------------------------------------- 65536 features
def big_cases(rng):
    nf = 65536
    xy = rng.uniform(0, 750, (nf, 2))
    cam = np.ones(nf, np.int32)
    cam[[0, nf - 1, 1, nf - 2]] = 0
    xy[[0, nf - 1, 1, nf - 2]] = [(100, 100), (103, 100), (400, 300), (403, 300)]
    fd = rng.integers(0, 256, (nf, 32), dtype=np.uint8)
    fd[[0, nf - 1, 1, nf - 2]] = weight_rows([9, 5, 9, 5])
    out = []
    for assigned_last in (0, 1):
        asg = np.zeros(nf, np.uint8)
        asg[nf - 1] = assigned_last
        F = frame(keys_of(xy), fd, cam=cam, size=(754, 480), nr_cams=2, assigned=asg)
        P = probes([101.5, 101.5, 401.5, 401.5, 100, 600, 300, 103], [100, 100, 300, 300, 100, 400, 200, 100], [2, 2, 2, 2, 0.5, 40, 300, 0], np.zeros((8, 32), np.uint8),
                   cam=[0, 0, 0, 0, 0, 1, 1, 0])
        for rule in (1, 2, 3, "best"):
            c = case("big/assigned%d/r%s" % (assigned_last, rule), "big", rule, F, P, nnratio=0.9)
            if rule == 3:
                c["probes"] = dict(P, lo=np.zeros(8, np.int32), hi=np.zeros(8, np.int32))
            out.append(c)
        out.append(as_rule0(out[-4], "big/assigned%d/r0" % assigned_last, th=0.5))
    return out


# ---------------------------------------------------------------------------------------------- rule 3 steals
def steal_cases():
    """targets T0..T3, one feature each.  Probe distances to a target are set by the probe's weight; fillers look at empty space."""
    xy = [(50, 50), (150, 50), (250, 50), (350, 50), (450, 50)]
    F = frame(keys_of(xy), np.zeros((5, 32), np.uint8), size=(754, 480))
    n = 200
    px, py, w = np.full(n, 600.0), np.full(n, 400.0), np.zeros(n, np.int64)
    plan = {
        0: (0, 30), 1: (0, 20), 2: (0, 10), 3: (0, 5), 4: (0, 5), 5: (0, 30),           # T0: stolen three times in a row, an equal distance does not steal
        10: (1, 40), 70: (1, 30), 130: (1, 20), 199: (1, 21),                            # T1: steals across rounds
        20: (2, 64), 21: (2, 65), 22: (2, 63),                                           # T2: TH_LOW and TH_LOW + 1, then a steal inside the round
        63: (3, 12), 64: (3, 11), 127: (3, 10), 128: (3, 9),                             # T3: steals across the round boundaries
        30: (4, 3), 31: (4, 3), 32: (4, 2), 33: (4, 4),                                  # T4
    }
    for p, (t, d) in plan.items():
        px[p], py[p], w[p] = xy[t][0], xy[t][1], d
    P = probes(px, py, 5.0, weight_rows(w), 0, 0)
    return [case("steal/r3", "steal", 3, F, P, nnratio=0.9, min_steals=3)]


# ---------------------------------------------------------------------------------------------- empty sides
def empty_cases(rng):
    F = frame(keys_of(rng.uniform(5, 120, (20, 2))), rng.integers(0, 256, (20, 32), dtype=np.uint8))
    F0 = frame(keys_of([]), np.zeros((0, 32), np.uint8))
    P = probes(rng.uniform(5, 120, 10), rng.uniform(5, 90, 10), 20.0, rng.integers(0, 256, (10, 32), dtype=np.uint8))
    P0 = probes(np.zeros(0), np.zeros(0), 1.0, np.zeros((0, 32), np.uint8))
    out = []
    for rule in (1, 2, 3, "best", "best_taken"):
        out.append(case("empty/nproj0/r%s" % rule, "empty", rule, F, P0))
        out.append(case("empty/nfeat0/r%s" % rule, "empty", rule, F0, P))
    out.append(as_rule0(out[0], "empty/nproj0/r0", th=1.0))
    out.append(as_rule0(out[1], "empty/nfeat0/r0", th=1.0))
    return out


_cases = None


def cases():
    """the case table, built once (seeded) and shared; nobody writes to it"""
    global _cases
    if _cases is None:
        rng = np.random.default_rng(20260)
        _cases = (geometry_cases(rng) + decision_cases(rng) + order_cases(rng) + cluster_cases(rng) + chain_cases() + collision_cases(rng) + big_cases(rng)
                  + steal_cases() + empty_cases(rng))
        names = [c["name"] for c in _cases]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return _cases
