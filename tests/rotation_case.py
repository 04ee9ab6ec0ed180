"""Every stage of the covisibility store in rotation on ONE store (tests/test_gpu_covis_rotation.py and its _cpu twin): the cases and the sequence of calls.

The stages share the per-point scratch of the store (csrc/mcs_covis.h: mult, key and the level counters are clean between calls) and the device code that
walks a row; no single-stage suite hands a store from one stage to the next.  rotate() is the sequence, written once against cull_pack.CullBoth's interface;
model_only() answers the device's part from the models, so the _cpu twin runs the very same sequence and asserts that it is not vacuous.

A case: 7 keyframes of L features each, one of them erased again after it was filled (its slot keeps a stale row), so 6 live keyframes and one hole; point ids
below 600; descriptors of 32 bytes with masks.  L = 1: one component of one 16-byte load; L = 5: two loads, the second with one entry and three of padding;
L = 257: 65 loads, so lane 0 of the wave makes a second trip.

What a case of 6 live keyframes can show.  A keyframe is culled when more than nine tenths of its counted features have five OTHER observers, i.e. are held by
every other live keyframe.  A point of the culled keyframe's row goes bad when two or fewer observers are left, so it was NOT one of those features: the row
needs at least ten redundant features beside it (10 > 0.9 * 11).  Rows of fewer than 11 features (L = 1, L = 5) therefore cannot lose a point through
mcs_covis_cull_keyframes, whatever the store holds; there the bad points come from mcs_covis_cull_points alone."""
import numpy as np

import covis_model as M
import cull_model as CM
import mappoint_model as MM
from cull_pack import CullBoth

LENGTHS = [1, 5, 257]
KIDS = [2, 5, 7, 11, 12, 20, 23]
HOLE = 7
A, B = 5, 12                                                      # the redundant keyframe, and the one that is not redundant once A is gone
MAX_PTS = 600
UNHELD, BAD0, BAD1 = 590, 400, 401                                # a point that no row holds; two points that are bad from the start
DIM = 32
SCALES = np.array([1.2 ** i for i in range(8)])


class Case:
    pass


def _rows(L, rng):
    """-> (rows, octaves, rare points): every live keyframe holds the core points, so A's features are redundant until one keyframe is gone"""
    live = [k for k in KIDS if k != HOLE]
    if L == 1:
        return {k: [0] for k in KIDS}, {k: [3] for k in KIDS}, []
    if L == 5:
        rows = {2: [0, 1, 2, 3, -1], 5: [0, 1, 0, BAD0, -1], 7: [0, 1, 2, 3, 4], 11: [1, 0, 2, 2, 4], 12: [0, -1, 1, 3, 5], 20: [2, 0, 1, BAD0, 3],
                23: [1, 3, 0, -1, 2]}
        return rows, {k: [3] * 5 for k in KIDS}, []
    ncore, rare = 240, list(range(300, 306))
    rows, octs = {}, {}
    others = [k for k in live if k != A]
    for k in KIDS:
        row = np.full(L, -1, np.int64)
        row[:ncore] = rng.permutation(ncore)
        if k == A:
            row[ncore:ncore + 6] = rare                            # A and two others hold a rare point: it goes bad with A
            row[ncore + 6:ncore + 8] = [BAD0, BAD1]
            row[ncore + 10:ncore + 14] = row[rng.integers(0, ncore, 4)]   # repeats: counted per feature, observed once
            o = rng.choice([3, 4], L)
            o[rng.permutation(ncore)[:5]] = 1                      # too fine for observers at level 3 and above: rejected by the octave test alone
        else:
            row[rng.permutation(ncore)[:1]] = -1                   # one core point loses this observer
            row[ncore:ncore + 6] = 310 + 10 * KIDS.index(k) + np.arange(6)   # points of its own
            row[ncore + 6:ncore + 9] = row[rng.integers(0, ncore, 3)]
            row[ncore + 9] = BAD1
            o = rng.integers(2, 5, L)
        rows[k], octs[k] = row, o
    for j, p in enumerate(rare):                                    # two further observers each, in the free tail of their rows
        for i in range(2):
            k = others[(j + i) % len(others)]
            free = np.flatnonzero(rows[k][ncore + 10:] < 0)[0] + ncore + 10
            rows[k][free] = p
    rows = {k: [int(p) for p in v] for k, v in rows.items()}
    return rows, {k: [int(x) for x in v] for k, v in octs.items()}, rare


def make_case(L, seed=None):
    rng = np.random.default_rng(100 + L if seed is None else seed)
    c = Case()
    c.L = L
    c.rows, c.octaves, c.rare = _rows(L, rng)
    assert all(len(r) == L for r in c.rows.values())
    c.poses = {k: rng.normal(0, 2, 3) for k in KIDS}
    c.desc = {k: rng.integers(0, 256, (L, DIM), dtype=np.uint8) for k in KIDS}
    c.mask = {k: rng.integers(0, 256, (L, DIM), dtype=np.uint8) | 0x11 for k in KIDS}
    c.bad_pts = [BAD0, BAD1]
    live = [k for k in KIDS if k != HOLE]
    held = sorted(set(p for k in live for p in c.rows[k] if p >= 0))
    # ---- the lists of the calls
    pts = [int(p) for p in rng.permutation(held)[:40]] + c.rare[:3] + [BAD0, UNHELD]
    pts = list(dict.fromkeys([0] + pts))                           # distinct; point 0 is held by every keyframe at every L
    first_obs = {p: next((k for k in live if p in c.rows[k]), live[0]) for p in pts}
    ref = [first_obs[p] for p in pts]
    ref[-1] = HOLE                                                  # an erased keyframe: status 2
    c.up_ids, c.up_ref, c.up_pos = pts, ref, rng.normal(0, 5, (len(pts), 3))
    c.cull1 = ([A, B], [0, 0])
    c.conn = [2, B, 23]
    recent = list(dict.fromkeys([UNHELD, 0, BAD0] + [int(p) for p in rng.permutation(held)[:25]] + c.rare[3:6]))
    c.recent = recent
    c.cur = 24
    c.found = [1 if i % 3 == 0 else 9 for i in range(len(recent))]  # every third point lies below the found ratio
    c.visible = [10] * len(recent)
    c.first = [int(v) for v in rng.integers(20, 25, len(recent))]
    c.obs_ids = sorted(set(held) | {UNHELD, BAD0, BAD1})
    c.frame = [int(p) for p in (held * 8)[:max(8, min(6 * len(held), 300))]] + [-1, BAD0]
    c.frame_t = (0.3, -0.2, 0.1)
    c.cull2 = ([23, 2, 20, 11], [0, 1, 0, 0])
    return c


class Rotation(CullBoth):
    """CullBoth with descriptors and mcs_covis_update_points; `d` needs set_descriptors() and update_points() beside cull_pack.CullDev's calls"""

    def __init__(self, d):
        self.m, self.d = M.Store(), d
        self.m.octaves = {}
        self.desc, self.mask = {}, {}

    def set_keyframe(self, kid, points):
        if kid in self.m.rows and len(self.m.rows[kid]) != len(points):
            self.desc.pop(kid, None); self.mask.pop(kid, None)
        super().set_keyframe(kid, points)

    def set_descriptors(self, kid, desc, mask):
        self.desc[kid], self.mask[kid] = np.array(desc, np.uint8), np.array(mask, np.uint8)
        assert self.d.set_descriptors(kid, desc, mask) == 0

    def erase(self, kid):
        super().erase(kid)
        self.desc.pop(kid, None); self.mask.pop(kid, None)

    def map_store(self):
        ms = MM.MapStore(self.m)
        ms.octaves, ms.desc, ms.mask, ms.dim, ms.masks = self.m.octaves, self.desc, self.mask, DIM, True
        return ms

    def check_update_points(self, ids, pos, ref, where=""):
        """one mcs_covis_update_points against tests/mappoint_model.py over the pack's own rows, octaves, poses and flags, bit for bit"""
        n = len(ids)
        d0 = np.full((n, DIM), 0xA5, np.uint8)
        m0 = np.full((n, DIM), 0x5A, np.uint8)
        want = MM.update_points(self.map_store(), ids, pos, ref, SCALES, d0, m0, max_points=MAX_PTS)
        got = self.d.update_points(ids, pos, ref, SCALES, d0, m0)
        assert set(got) == set(want)
        for k in want:
            w = np.ascontiguousarray(want[k])
            g = np.ascontiguousarray(got[k]).astype(w.dtype, copy=False).reshape(w.shape)
            assert g.tobytes() == w.tobytes(), (where, k, [(i, a, b) for i, (a, b) in enumerate(zip(g.tolist(), w.tolist())) if str(a) != str(b)][:4])
        return want


class _ModelDev:
    """the device's side answered by the models from the pack's own model store: the sequence then runs without a GPU"""

    def __init__(self):
        self.b = None

    def _ok(self, *a, **k):
        return 0

    set_keyframe = set_pose = erase = set_bad = set_points_bad = set_octaves = set_descriptors = _ok

    def update_reference(self, frame_points, frame_t, cap):
        r = M.update_reference(self.b.m, frame_points, frame_t)
        r["n_points"] = len(r["local_points"])
        r["local_points"] = r["local_points"][:cap]
        return r

    def update_connections(self, ids):
        return [M.update_connections(self.b.m, k) for k in ids]

    def cull_keyframes(self, ids, not_erase, cap):
        r = CM.keyframe_culling(self.b.m, self.b.m.octaves, ids, not_erase)
        return dict(verdict=r["verdict"], n_mps=r["n_mps"], n_redundant=r["n_redundant"], bad_points=r["bad_points"][:cap], n_bad_points=len(r["bad_points"]))

    def observations(self, ids):
        return CM.observations(self.b.m, ids)

    def cull_points(self, cur, ids, found, visible, first):
        return CM.map_point_culling(self.b.m, cur, ids, found, visible, first)["verdict"]

    def update_points(self, ids, pos, ref, scales, d0, m0):
        return MM.update_points(self.b.map_store(), ids, pos, ref, scales, d0, m0, max_points=MAX_PTS)


def model_only():
    d = _ModelDev()
    b = Rotation(d)
    d.b = b
    return b


def load(b, c):
    """the case into the pair: seven keyframes with octaves and descriptors, the hole, poses and the points that are bad from the start"""
    for k in KIDS:
        b.set_keyframe(k, c.rows[k])
        b.set_octaves(k, c.octaves[k])
        b.set_descriptors(k, c.desc[k], c.mask[k])
    b.set_pose(KIDS, [c.poses[k] for k in KIDS])
    b.erase(HOLE)
    b.set_points_bad(c.bad_pts)


def rotate(b, c):
    """the rotation; every call is compared with its model inside the check.  -> what the models said, for the assertions on vacuity, and the final local map"""
    log = {}
    log["up1"] = b.check_update_points(c.up_ids, c.up_pos, c.up_ref, "update_points 1")
    log["cull1"] = b.check_cull(*c.cull1, where="cull_keyframes 1", erase=False)   # the culled keyframe stays in its slot, bad: its rows still count
    log["conn"] = b.check_connections([k for k in c.conn if k in b.m.rows], "update_connections")
    log["cullpts"] = b.check_cull_points(c.cur, c.recent, c.found, c.visible, c.first, "cull_points")
    log["up2"] = b.check_update_points(c.up_ids, c.up_pos, c.up_ref, "update_points 2")
    b.check_observations(c.obs_ids, "observations")
    log["ref"] = b.check_reference(c.frame, c.frame_t, where="update_reference")
    log["cull2"] = b.check_cull(*c.cull2, where="cull_keyframes 2")
    log["final"] = b.check_reference(c.frame, c.frame_t, where="the final update_reference")
    return log


def assert_not_vacuous(c, log):
    """on the MODELS' results alone"""
    v1 = log["cull1"]["verdict"]
    assert v1 == [1, 0], v1                                         # A is redundant and culled; B, with one observer fewer, is not
    by_points = [p for p, v in zip(c.recent, log["cullpts"]["verdict"]) if v in (2, 3)]
    assert 2 in log["cullpts"]["verdict"] and len(by_points) > 0    # below the found ratio
    by_keyframes = log["cull1"]["bad_points"] + log["cull2"]["bad_points"]
    if c.L >= 11:                                                   # the module's docstring: shorter rows cannot lose a point that way
        assert len(by_keyframes) > 0 and set(by_keyframes) <= set(c.rare)
    else:
        assert by_keyframes == []
    for key in ("up1", "up2"):
        st, nd = log[key]["status"], log[key]["n_desc"]
        assert ((st == 0) & (nd > 0)).any() and (st != 0).any(), (key, st.tolist(), nd.tolist())   # a descriptor chosen, and an entry refused
    s1, s2 = log["up1"]["status"], log["up2"]["status"]
    assert (s1 != s2).any() and (log["up1"]["n_desc"] != log["up2"]["n_desc"]).any()   # the culls in between changed what a refresh finds
    assert len(log["final"]["local_kfs"]) > 0 and len(log["final"]["local_points"]) > 0
    assert any(r["ordered"] for r in log["conn"])


def fresh_copy(b, d):
    """a pair on the fresh device store `d` that holds the model's state of `b` (rows, octaves, poses, flags): what a store that never ran a call holds"""
    f = Rotation(d)
    ids = sorted(b.m.rows)
    for k in ids:
        f.set_keyframe(k, b.m.rows[k])
        f.set_octaves(k, b.m.octaves[k])
    f.set_pose(ids, [b.m.t[k] for k in ids])
    for k in ids:
        if b.m.kf_bad[k]:
            f.set_bad(k)
    f.set_points_bad(sorted(b.m.pt_bad))
    return f
