"""The raw C ABI of mcs_triangulate_matches / mcs_create_new_map_points over the keyframes of tests/newpoints_model.py: host-kind calls on numpy arrays,
device-kind calls on hipMalloc'ed copies (gpu_common.DevBuf).  The parity tests drive the library without keyframe objects."""
import ctypes as C

import numpy as np

import newpoints_model as M


class Mem:
    """arrays of one call in host or device memory; .p(arr) -> pointer value, .out(arr) registers an output to read back"""

    def __init__(self, G, device):
        self.G, self.device, self.keep = G, device, []

    def p(self, arr):
        if arr is None:
            return None
        arr = np.ascontiguousarray(arr)
        if self.device:
            b = self.G.DevBuf(arr)
            self.keep.append(b)
            return b.ptr.value
        self.keep.append(arr)
        return arr.ctypes.data

    def out(self, arr):
        """-> (pointer, reader)"""
        if self.device:
            b = self.G.DevBuf(arr)
            self.keep.append(b)
            return b.ptr.value, b.read
        self.keep.append(arr)
        return arr.ctypes.data, (lambda: arr)


def ocam(pkg, cam):
    """mcs_ocam of a camera dict.  Two keys only the hostile cases carry: "invP_pad" fills invP past invP_deg (the library must not read it),
    "invP_deg" declares a degree other than the number of coefficients given"""
    o = pkg.make_ocam(cam)
    if "invP_pad" in cam:
        for k in range(len(cam["invP"]), pkg._capi.MAX_POLY):
            o.invP[k] = cam["invP_pad"]
    if "invP_deg" in cam:
        o.invP_deg = cam["invP_deg"]
    return o


def geom(pkg, mem, kf, with_mp, mp=None):
    """mp: explicit (mp_pos [n_mp, 3], mp_cam [n_mp]) instead of the positions / cameras of the features that hold a map point (default: kf.mp)"""
    cap = pkg._capi
    ocs = (cap.Ocam * kf.nr)(*[ocam(pkg, c) for c in kf.cams])
    g = cap.KfGeom()
    g.MtMc, g.MtMc_inv, g.M_t = mem.p(kf.MtMc.reshape(-1)), mem.p(kf.MtMc_inv.reshape(-1)), mem.p(kf.M_t.reshape(-1))
    g.cams = mem.p(np.frombuffer(ocs, np.uint8).copy())
    g.rays, g.keys, g.cam = mem.p(kf.rays), mem.p(kf.keys), mem.p(kf.cam)
    g.n, g.nr_cams = kf.n, kf.nr
    if with_mp:
        pos, cam = M.map_points(kf, mp)
        g.mp_pos, g.mp_cam, g.n_mp = mem.p(pos), mem.p(cam), len(cam)
    return g


def desc_set(pkg, mem, kf, g, valid=None):
    valid = (~kf.has_mp) if valid is None else valid
    return pkg._capi.DescSet(mem.p(kf.desc), mem.p(kf.mask), mem.p(np.ascontiguousarray(valid, np.uint8)), g.cam, kf.n, kf.desc.shape[1], 0, 0)


class Outputs:
    def __init__(self, pkg, mem, nsets, n1):
        rows = max(nsets * n1, 1)
        self.nsets, self.n1 = nsets, n1
        self.o = pkg._capi.NewPointsOut()
        self.rd = {}
        for name, arr in (("verdict", np.full(rows, -9, np.int32)), ("x3D", np.full(rows * 3, -7.0)), ("acc_count", np.full(nsets, -9, np.int32)),
                          ("acc_idx1", np.full(rows, -9, np.int32)), ("acc_idx2", np.full(rows, -9, np.int32)), ("acc_x3D", np.full(rows * 3, -7.0))):
            ptr, self.rd[name] = mem.out(arr)
            setattr(self.o, name, ptr)

    def read(self):
        ns, n1 = self.nsets, self.n1
        r = self.raw = {k: f() for k, f in self.rd.items()}   # the whole arrays, sentinels included
        out = []
        for s in range(ns):
            k = int(r["acc_count"][s])
            out.append(dict(verdict=r["verdict"][s * n1:(s + 1) * n1], x3D=r["x3D"][3 * s * n1:3 * (s + 1) * n1].reshape(-1, 3),
                            idx1=r["acc_idx1"][s * n1:s * n1 + k], idx2=r["acc_idx2"][s * n1:s * n1 + k],
                            acc_x3D=r["acc_x3D"][3 * s * n1:3 * (s * n1 + k)].reshape(-1, 3)))
        return out


def triangulate(pkg, ctx, G, pairs, matches, device=False, skipped=None, cosThresh=M.COS_THRESH, maxDIST=M.MAX_DIST, raw=False):
    """mcs_triangulate_matches over [(kf1, kf2)] pairs with matches [nsets][n1] -> per pair dicts (raw: and the whole output arrays by name)"""
    cap = pkg._capi
    mem = Mem(G, device)
    ns, n1 = len(pairs), pairs[0][0].n
    shared = {}
    g1 = (cap.KfGeom * ns)()
    g2 = (cap.KfGeom * ns)()
    for s, (a, b) in enumerate(pairs):
        if id(a) not in shared:
            shared[id(a)] = geom(pkg, mem, a, False)
        g1[s], g2[s] = shared[id(a)], geom(pkg, mem, b, False)
    m12 = mem.p(np.ascontiguousarray(np.concatenate(matches), np.int32))
    sk = None if skipped is None else mem.p(np.ascontiguousarray(skipped, np.uint8))
    outs = Outputs(pkg, mem, ns, n1)
    pkg.check(pkg.lib().mcs_triangulate_matches(ctx.h, ns, g1, g2, m12, sk, cosThresh, maxDIST, int(device), C.byref(outs.o)))
    if device:
        ctx.synchronize()
    res = outs.read()
    return (res, outs.raw) if raw else res


def chain(pkg, ctx, G, kf1, neigh, device=False, check_ori=False, valid1=None, E=None, K=16, cosThresh=M.COS_THRESH, maxDIST=M.MAX_DIST, expect=0):
    """mcs_create_new_map_points -> (per neighbour dicts incl. match12 / nmatches / fallbacks / baseline / median / skipped, final valid1)"""
    cap = pkg._capi
    mem = Mem(G, device)
    ns, n1 = len(neigh), kf1.n
    g1 = geom(pkg, mem, kf1, False)
    s1 = desc_set(pkg, mem, kf1, g1, valid1)
    g2 = (cap.KfGeom * ns)()
    s2 = (cap.DescSet * ns)()
    for s, kf in enumerate(neigh):
        g2[s] = geom(pkg, mem, kf, True)
        s2[s] = desc_set(pkg, mem, kf, g2[s])
    outs = Outputs(pkg, mem, ns, n1)
    pm, rm = mem.out(np.full(max(ns * n1, 1), -9, np.int32))
    pn, rn = mem.out(np.full(ns, -9, np.int32))
    pf, rf = mem.out(np.full(ns, -9, np.int32))
    pb, rb = mem.out(np.full(ns, -7.0))
    pd, rdm = mem.out(np.full(ns, -7.0))
    ps, rs = mem.out(np.full(ns, 9, np.uint8))
    pv, rv = mem.out(np.full(max(n1, 1), 9, np.uint8))
    Ep = None if E is None else mem.p(np.ascontiguousarray(E, np.float64))
    pitch = 0 if E is None else 9 * kf1.nr * kf1.nr
    rc = pkg.lib().mcs_create_new_map_points(ctx.h, ns, C.byref(g1), C.byref(s1), g2, s2, Ep, pitch, kf1.desc.shape[1], K, int(check_ori), cosThresh, maxDIST,
                                             int(device), pm, pn, pf, pb, pd, ps, pv, C.byref(outs.o))
    if expect:
        assert rc == expect, rc
        return None, None
    pkg.check(rc)
    if device:
        ctx.synchronize()
    res = outs.read()
    m12, nm, fb, bl, md, sk = rm(), rn(), rf(), rb(), rdm(), rs()
    for s in range(ns):
        res[s].update(match12=m12[s * n1:(s + 1) * n1], nmatches=int(nm[s]), fallbacks=int(fb[s]), baseline=float(bl[s]), median=float(md[s]), skipped=bool(sk[s]))
    return res, rv()[:n1].astype(bool)


def same_bits(a, b):
    """doubles equal bit for bit (so -0.0 != 0.0); a NaN equals any NaN: which sign and payload an invalid operation produces is the hardware's choice
    (x86 gives the negative default NaN, the GPU the positive one), not the arithmetic's"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    ok = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        print("first differing double at %s: %r (%016x) vs %r (%016x)" % (i, a[i], a.view(np.uint64)[i], b[i], b.view(np.uint64)[i]))
    return bool(ok.all())


def compare(got, want, label, with_search=True):
    """device result of one pair against the model's: everything equal, doubles bit for bit"""
    assert np.array_equal(got["verdict"], want["verdict"]), "%s: verdicts %s" % (label, np.flatnonzero(got["verdict"] != want["verdict"])[:8])
    assert np.array_equal(got["idx1"], want["idx1"]) and np.array_equal(got["idx2"], want["idx2"]), "%s: accepted lists" % label
    assert same_bits(got["x3D"], want["x3D"]), "%s: x3D bits" % label
    assert same_bits(got["acc_x3D"], want["acc_x3D"]), "%s: accepted x3D bits" % label
    if with_search:
        assert np.array_equal(got["match12"], want["match12"]), "%s: match12" % label
        assert got["nmatches"] == int((want["match12"] >= 0).sum()), "%s: nmatches" % label
        assert got["skipped"] == want["skipped"], "%s: skipped" % label
        assert same_bits([got["baseline"], got["median"]], [want["baseline"], want["median"]]), "%s: baseline / median" % label
