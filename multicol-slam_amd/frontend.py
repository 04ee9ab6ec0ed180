"""Host-side mirror of the reference's class surface for the hot path (same names, argument meaning and outputs):

  mdBRIEFextractorOct / ORBextractor   include/mdBRIEFextractorOct.h:335-421, include/cORBextractor.h:61-63
  cMultiFrame (extraction part)        include/cMultiFrame.h:62-162, src/cMultiFrame.cpp:92-216,342-353
  cORBmatcher (brute-force searches)   include/cORBmatcher.h:43-133, src/cORBmatcher.cpp:46-65,179-323,885-1155
  cORBmatcher (grid-window searches)   src/cORBmatcher.cpp:67-166,326-726,1990-2118
  cMultiCamSys_ (pose, projection)     src/cam_system_omni.cpp:92-133,168-198
  DescriptorDistance64[_Masked]        src/cORBmatcher.cpp:2438-2474
  cMultiKeyFrameDatabase               src/cMultiKeyFrameDatabase.cpp:43-329 (inverted file, relocalisation / loop candidates)
  cSim3Solver (+ cSim3SolverBatch)     src/cSim3Solver.cpp (the RANSAC of cLoopClosing::ComputeSim3, one round over many candidates per call)
  CreateNewMapPoints                   src/cLocalMapping.cpp:223-381 (the mapping thread's neighbour loop: search, triangulation and checks in one call)
  cMultiFrame.isInFrustum, SearchReferencePointsInFrustum   src/cMultiFrame.cpp:218-270, src/cTracking.cpp:953-1012 (the search step of TrackLocalMap in one call)
  cCovisibility, TrackLocalMapSearch   src/cTracking.cpp:1024-1123, src/cMultiKeyFrame.cpp:406-500 (local map and covisibility counts from a device-resident store)
  PoseOptimization[Batch]              src/cOptimizer.cpp:259-459 (the frame's pose, both g2o rounds in one call, a batch of frames per call)

Everything numeric runs in libmcs_hip.so on the GPU; this file only shapes inputs/outputs (numpy stands in for cv::Mat).
"""
import ctypes as C
import math

import numpy as np

from . import Context, Extractor
from ._capi import KP_DTYPE, MEM_DEVICE, MEM_HOST, MCS_ERR_CAPACITY, DescSet, KfdbDiag, check, lib, make_ocam, np_ptr

FRAME_GRID_ROWS, FRAME_GRID_COLS = 48, 64   # include/cMultiFrame.h

_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class cCamModelGeneral_:
    """Scaramuzza omni camera (include/cam_model_omni.h); holds the calibration and the level-0 mirror mask."""

    def __init__(self, cdeu0v0, p, invP, Iw, Ih, mirror_mask=None):
        c, d, e, u0, v0 = cdeu0v0
        self.calib = dict(c=c, d=d, e=e, u0=u0, v0=v0, p=list(p), invP=list(invP), width=int(Iw), height=int(Ih))
        self.ocam = make_ocam(self.calib)
        self._mask = mirror_mask

    @classmethod
    def from_dict(cls, cam, mirror_mask=None):
        return cls((cam["c"], cam["d"], cam["e"], cam["u0"], cam["v0"]), cam["p"], cam["invP"], cam["width"], cam["height"], mirror_mask)

    def GetWidth(self):
        return self.calib["width"]

    def GetHeight(self):
        return self.calib["height"]

    def GetMirrorMask(self, level=0):
        assert level == 0, "only level 0 is used by the extractor (src/cMultiFrame.cpp:138)"
        return self._mask


def _matx_mul(A, B):
    """cv::Matx product (s = 0; s += a(i,k) * b(k,j) in k order), so MtMc is rounded like the reference's."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.zeros((A.shape[0], B.shape[1]))
    for i in range(A.shape[0]):
        for j in range(B.shape[1]):
            acc = np.float64(0.0)
            for k in range(A.shape[1]):
                acc = acc + A[i, k] * B[k, j]
            out[i, j] = acc
    return out


def _inv_mat(M):
    """cConverter::invMat (src/cConverter.cpp:31-44): rigid inverse, t = -(R^T) * t."""
    M = np.asarray(M, np.float64)
    Rt = M[:3, :3].T.copy()
    t = _matx_mul(-Rt, M[:3, 3:4])[:, 0]
    out = np.eye(4)
    out[:3, :3] = Rt
    out[:3, 3] = t
    return out


def _hom2cayley(M):   # include/misc.h:171-202
    M = np.asarray(M, np.float64)
    R = M[:3, :3]
    Cm = (R - np.eye(3)) @ np.linalg.inv(R + np.eye(3))
    return np.array([-Cm[1, 2], Cm[0, 2], -Cm[0, 1], M[0, 3], M[1, 3], M[2, 3]])


class cMultiCamSys_:
    """Calibrations + poses of the rig (include/cam_system_omni.h): M_t = rig pose, M_c[c] = camera c in the rig frame."""

    def __init__(self, cam_models, M_c=None, M_t=None):
        self.cams = list(cam_models)
        self.M_c = [np.asarray(m, np.float64) for m in M_c] if M_c is not None else [np.eye(4) for _ in self.cams]
        self.Set_M_t(np.eye(4) if M_t is None else M_t)

    def Set_M_t(self, M_t_):   # src/cam_system_omni.cpp:184-198
        self.M_t = np.asarray(M_t_, np.float64).copy()
        self.M_t_inv = _inv_mat(self.M_t)
        self.MtMc = [_matx_mul(self.M_t, mc) for mc in self.M_c]
        self.MtMc_inv = [_inv_mat(m) for m in self.MtMc]

    def Get_M_c_min(self, c):   # the calibration's 6-vector where the rig was built from one (M_c_min), else hom2cayley(M_c[c]) (include/misc.h:171-202)
        if getattr(self, "M_c_min", None) is not None:
            return np.asarray(self.M_c_min[c], np.float64)
        return _hom2cayley(self.M_c[c])

    def GetPoseMin(self):
        return self.M_t_min.copy() if getattr(self, "M_t_min", None) is not None else _hom2cayley(self.M_t)

    def Set_M_t_from_min(self, M_t_minRep, MtMc=None, MtMc_inv=None):   # src/cam_system_omni.cpp:170-183; MtMc / MtMc_inv: as a device call built them
        from .io import cayley2hom
        self.M_t_min = np.asarray(M_t_minRep, np.float64).reshape(6).copy()
        self.M_t = cayley2hom(self.M_t_min)
        self.M_t_inv = _inv_mat(self.M_t)
        if MtMc is None:
            M_c = [cayley2hom(self.Get_M_c_min(c)) for c in range(len(self.cams))] if getattr(self, "M_c_min", None) is not None else self.M_c
            MtMc = [_matx_mul(self.M_t, mc) for mc in M_c]
            MtMc_inv = [_inv_mat(m) for m in MtMc]
        self.MtMc = [np.asarray(m, np.float64).reshape(4, 4).copy() for m in MtMc]
        self.MtMc_inv = [np.asarray(m, np.float64).reshape(4, 4).copy() for m in MtMc_inv]

    def world_to_cam(self, pts3, cam_idx, ctx=None):
        """Batched WorldToCamHom_fast + isPointInMirrorMask(u, v, 0) on the GPU -> (uv [n,2] float64, flags [n] uint8; bit0 = in mask,
        bit1 = behind the camera)."""
        pts3 = np.ascontiguousarray(pts3, np.float64).reshape(-1, 3)
        cam_idx = np.ascontiguousarray(cam_idx, np.int32)
        n = len(pts3)
        uv, flags = np.zeros((max(n, 1), 2)), np.zeros(max(n, 1), np.uint8)
        if n == 0:
            return uv[:0], flags[:0]
        nr = len(self.cams)
        M = np.ascontiguousarray(np.stack(self.MtMc_inv).reshape(nr, 16))
        ocs = (type(self.cams[0].ocam) * nr)(*[cm.ocam for cm in self.cams])
        masks = [cm.GetMirrorMask(0) for cm in self.cams]
        keep = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in masks]
        mp = (C.c_void_p * nr)(*[None if m is None else m.ctypes.data for m in keep])
        ctx = ctx or default_context()
        check(lib().mcs_world_to_cam(ctx.h, np_ptr(M), ocs, nr, mp if any(m is not None for m in keep) else None, np_ptr(pts3), np_ptr(cam_idx), n,
                                     MEM_HOST, np_ptr(uv), np_ptr(flags)))
        return uv[:n], flags[:n]

    def WorldToCamHom_fast(self, c, pt3):   # src/cam_system_omni.cpp:114-133
        uv, _ = self.world_to_cam(np.asarray(pt3, np.float64)[:3].reshape(1, 3), [c])
        return uv[0]

    def GetNrCams(self):
        return len(self.cams)

    def GetCamModelObj(self, c):
        return self.cams[c]


class mdBRIEFextractorOct:
    """Same 13 constructor arguments as the reference (include/mdBRIEFextractorOct.h:339-351)."""

    HARRIS_SCORE, FAST_SCORE = 0, 1

    def __init__(self, _nfeatures=1000, _scaleFactor=1.2, _nlevels=8, _edgeThreshold=25, _firstLevel=0, _scoreType=0, _patchSize=32,
                 _fastThreshold=20, _useAgast=False, _fastAgastType=2, _do_dBrief=False, _learnMasks=False, _descSize=32, ctx=None):
        self.kw = dict(nfeatures=_nfeatures, scaleFactor=_scaleFactor, nlevels=_nlevels, edgeThreshold=_edgeThreshold, firstLevel=_firstLevel,
                       scoreType=_scoreType, patchSize=_patchSize, fastThreshold=_fastThreshold, useAgast=int(_useAgast),
                       fastAgastType=_fastAgastType, do_dBrief=int(_do_dBrief), learnMasks=int(_learnMasks), descSize=_descSize)
        self.ctx = ctx or default_context()
        self._ex = {}

    def _extractor(self, w, h, batch):
        key = (w, h)
        ex = self._ex.get(key)
        if ex is None or ex.max_batch < batch:
            if ex is not None:
                ex.close()
            ex = Extractor(self.ctx, w, h, max_batch=max(batch, 1), **self.kw)
            self._ex[key] = ex
        return ex

    def __call__(self, image, mask, camModel):
        """operator()(image, mask, keypoints, camModel, descriptors, descriptorMasks) -> (keypoints, descriptors, descriptorMasks)."""
        if image is None or image.size == 0:
            return np.zeros(0, KP_DTYPE), None, None     # empty image -> silent return (:1252-1253)
        assert image.dtype == np.uint8 and image.ndim == 2   # assert(image.type() == CV_8UC1) (:1256)
        h, w = image.shape
        ex = self._extractor(w, h, 1)
        cams = None if camModel is None else [camModel.ocam]
        kps, d, dm, _ = ex.extract_host([image], None if mask is None else [mask], cams, want_rays=False)[0]
        if len(kps) == 0:
            return kps, None, None                        # _descriptors.release() (:1270-1274)
        return kps, d, dm

    def extract_rig(self, images, masks, cam_models):
        """All cameras of a multi-frame in ONE device batch (the GPU analogue of the reference's omp loop over cameras)."""
        h, w = images[0].shape
        ex = self._extractor(w, h, len(images))
        return ex.extract_host(images, masks, [c.ocam for c in cam_models], want_rays=True)

    def GetLevels(self):
        return self.kw["nlevels"]

    def GetScaleFactor(self):
        return float(np.float32(self.kw["scaleFactor"]))   # the member is the double of the FLOAT ctor argument

    def GetMasksLearned(self):
        return bool(self.kw["learnMasks"])

    def GetDescriptorSize(self):
        return self.kw["descSize"]


class ORBextractor(mdBRIEFextractorOct):
    """include/cORBextractor.h (declared but never built in the reference): the extractor in ORB mode."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, scoreType=1, fastTh=20, ctx=None):
        super().__init__(nfeatures, scaleFactor, nlevels, 25, 0, scoreType, 32, fastTh, False, 2, False, False, 32, ctx=ctx)

    def __call__(self, image, mask):
        kps, d, _ = super().__call__(image, mask, None)
        return kps, d


class cMultiFrame:
    """Extraction part of cMultiFrame::cMultiFrame (src/cMultiFrame.cpp:92-216): public fields the matcher/tracker read."""

    nNextId = 0

    def __init__(self, images, timeStamp, extractor, voc, camSystem, imgCnt=0):
        nrCams = camSystem.GetNrCams()
        self.images, self.mTimeStamp, self.camSystem, self.imgCnt = images, timeStamp, camSystem, imgCnt
        self.mpORBvocabulary, self.mBowVec, self.mFeatVec = voc, None, None
        ex0 = extractor[0] if isinstance(extractor, (list, tuple)) else extractor
        cams = [camSystem.GetCamModelObj(c) for c in range(nrCams)]
        masks = [cm.GetMirrorMask(0) for cm in cams]
        res = ex0.extract_rig(list(images), None if any(m is None for m in masks) else masks, cams)
        self.mDescriptors = [r[1] for r in res]
        self.mDescriptorMasks = [r[2] for r in res]
        self.N = [len(r[0]) for r in res]
        self.totalN = int(sum(self.N))
        self.mvKeys = np.concatenate([r[0] for r in res]) if self.totalN else np.zeros(0, KP_DTYPE)
        self.mvKeysRays = np.concatenate([r[3] for r in res]) if self.totalN else np.zeros((0, 3))
        self.keypoint_to_cam = np.concatenate([np.full(n, c, np.int32) for c, n in enumerate(self.N)]) if self.totalN else np.zeros(0, np.int32)
        self.cont_idx_to_local_cam_idx = np.concatenate([np.arange(n, dtype=np.int32) for n in self.N]) if self.totalN else np.zeros(0, np.int32)
        self.mnMinX, self.mnMinY = [0] * nrCams, [0] * nrCams
        self.mnMaxX = [cm.GetWidth() for cm in cams]
        self.mnMaxY = [cm.GetHeight() for cm in cams]
        self.mfGridElementWidthInv = [FRAME_GRID_COLS / float(self.mnMaxX[c] - self.mnMinX[c]) for c in range(nrCams)]
        self.mfGridElementHeightInv = [FRAME_GRID_ROWS / float(self.mnMaxY[c] - self.mnMinY[c]) for c in range(nrCams)]
        self.mGrids = [[[[] for _ in range(FRAME_GRID_ROWS)] for _ in range(FRAME_GRID_COLS)] for _ in range(nrCams)]
        for i in range(self.totalN):   # serial flatten + grid fill (:167-184)
            c = int(self.keypoint_to_cam[i])
            ok, gx, gy = self.PosInGrid(c, self.mvKeys[i])
            if ok:
                self.mGrids[c][gx][gy].append(i)
        self.mvbOutlier = [False] * self.totalN
        self.mvpMapPoints = [None] * self.totalN
        self.mnId = cMultiFrame.nNextId
        cMultiFrame.nNextId += 1
        self.mnScaleLevels = ex0.GetLevels()
        self.mfScaleFactor = ex0.GetScaleFactor()
        self.mvScaleFactors, self.mvLevelSigma2 = [1.0], [1.0]
        for i in range(1, self.mnScaleLevels):
            self.mvScaleFactors.append(self.mvScaleFactors[i - 1] * self.mfScaleFactor)
            self.mvLevelSigma2.append(self.mvScaleFactors[i] * self.mvScaleFactors[i])
        self.mvInvLevelSigma2 = [1 / s for s in self.mvLevelSigma2]
        self.masksLearned = ex0.GetMasksLearned()
        self.descDimension = ex0.GetDescriptorSize()

    def PosInGrid(self, cam, kp):   # src/cMultiFrame.cpp:342-353 (cvRound, not floor; bins 64 / 48 are dropped)
        posX = int(np.rint((float(kp["x"]) - self.mnMinX[cam]) * self.mfGridElementWidthInv[cam]))
        posY = int(np.rint((float(kp["y"]) - self.mnMinY[cam]) * self.mfGridElementHeightInv[cam]))
        if posX < 0 or posX >= FRAME_GRID_COLS or posY < 0 or posY >= FRAME_GRID_ROWS:
            return False, posX, posY
        return True, posX, posY

    def ComputeBoW(self):   # src/cMultiFrame.cpp:356-363 (voc = the cORBVocabulary given to the constructor)
        if not getattr(self, "mBowVec", None):
            self.mBowVec, self.mFeatVec = self.mpORBvocabulary.transform(self.all_descriptors(), 4)

    def isInFrustum(self, cam, pMP, viewingCosLimit=0.3, ctx=None):
        """bool cMultiFrame::isInFrustum(int cam, cMapPoint *pMP, double viewingCosLimit) (src/cMultiFrame.cpp:218-270): one slot through mcs_frustum.
        Writes mbTrackInView[cam] and, if in view, mTrackProjX/Y[cam], mnTrackScaleLevel[cam], mTrackViewCos[cam] onto pMP.  viewingCosLimit is not applied,
        as in the reference (:249-250)."""
        pts = _local_points([pMP], None)
        pts["flags"][:] = 0                       # the function itself does not look at isBad() / mnLastFrameSeen
        rv, keep = _rig_view(self.camSystem, cams=[cam])
        st = dict(in_view=np.zeros(1, np.uint8), proj_x=np.zeros(1), proj_y=np.zeros(1), level=np.zeros(1, np.int32), view_cos=np.zeros(1))
        vis, ntm = np.zeros(1, np.int32), np.zeros(1, np.int32)
        sc = np.ascontiguousarray(self.mvScaleFactors, np.float64)
        from ._capi import TrackState
        ts = TrackState(*[np_ptr(st[k]) for k in ("in_view", "proj_x", "proj_y", "level", "view_cos")])
        check(lib().mcs_frustum((ctx or default_context()).h, C.byref(pts["struct"]), C.byref(rv), np_ptr(sc), len(sc), C.byref(ts), MEM_HOST,
                                np_ptr(vis), np_ptr(ntm)))
        pMP.mbTrackInView[cam] = bool(st["in_view"][0])
        if st["in_view"][0]:
            pMP.mTrackProjX[cam], pMP.mTrackProjY[cam] = float(st["proj_x"][0]), float(st["proj_y"][0])
            pMP.mnTrackScaleLevel[cam], pMP.mTrackViewCos[cam] = int(st["level"][0]), float(st["view_cos"][0])
        return bool(st["in_view"][0])

    # flat (all cameras concatenated) descriptor views, the row order of mvKeys
    def all_descriptors(self):
        return np.concatenate(self.mDescriptors) if self.totalN else np.zeros((0, self.descDimension), np.uint8)

    def all_masks(self):
        return np.concatenate(self.mDescriptorMasks) if self.totalN else np.zeros((0, self.descDimension), np.uint8)


class cMultiKeyFrame:
    """Thin keyframe view: the accessors the brute-force searches use (src/cMultiKeyFrame.cpp:54,77,356-364)."""

    nNextId = 0

    def __init__(self, F):
        self.mnId = cMultiKeyFrame.nNextId          # src/cMultiKeyFrame.cpp:38-45
        cMultiKeyFrame.nNextId += 1
        self.mnFrameId = getattr(F, "mnId", None)
        self.camSystem = F.camSystem
        self.mDescriptors, self.mDescriptorMasks = F.mDescriptors, F.mDescriptorMasks   # shallow copies like cv::Mat
        self.mvKeys, self.mvKeysRays = F.mvKeys, F.mvKeysRays
        self.keypoint_to_cam, self.cont_idx_to_local_cam_idx = F.keypoint_to_cam, F.cont_idx_to_local_cam_idx
        self.mvpMapPoints = list(F.mvpMapPoints)
        self._d, self._m = F.all_descriptors(), F.all_masks()
        self.mBowVec, self.mFeatVec = getattr(F, "mBowVec", None), getattr(F, "mFeatVec", None)
        self.mvpOrderedConnectedKeyFrames = []
        self.mvLevelSigma2 = list(getattr(F, "mvLevelSigma2", [1.0]))
        self.mvInvLevelSigma2 = list(getattr(F, "mvInvLevelSigma2", [1 / s for s in self.mvLevelSigma2]))

    def GetSigma2(self, nLevel=1):                  # include/cMultiKeyFrame.h:162-163
        return self.mvLevelSigma2[nLevel]

    def GetInvSigma2(self, nLevel=1):               # include/cMultiKeyFrame.h:165-166
        return self.mvInvLevelSigma2[nLevel]

    def GetKeyPoint(self, idx):
        return self.mvKeys[idx]

    def GetBestCovisibilityKeyFrames(self, N):      # src/cMultiKeyFrame.cpp:231-240
        return list(self.mvpOrderedConnectedKeyFrames[:N])

    def GetMapPointMatches(self):
        return self.mvpMapPoints

    def GetFeatureVector(self):
        return self.mFeatVec

    def GetKeyPoints(self):
        return self.mvKeys

    def GetKeyPointsRays(self):
        return self.mvKeysRays

    def GetCameraCenter(self):                      # src/cMultiKeyFrame.cpp:156-162: Hom2T(M_t)
        return self.camSystem.M_t[:3, 3].copy()

    def ComputeSceneMedianDepth(self, q=2):         # src/cMultiKeyFrame.cpp:747-778 (host restatement; the device computes it inside CreateNewMapPoints)
        z = []
        for i, mp in enumerate(self.mvpMapPoints):
            if mp is not None:
                x4 = np.append(np.asarray(mp.GetWorldPos(), np.float64)[:3], 1.0).reshape(4, 1)
                z.append(_matx_mul(self.camSystem.MtMc_inv[int(self.keypoint_to_cam[i])], x4)[2, 0])
        z.sort()
        return z[(len(z) - 1) // q]                 # the reference indexes an empty vector when the keyframe holds no map point; here: IndexError


def _good(mp):
    return mp is not None and not (hasattr(mp, "isBad") and mp.isBad())


class cORBmatcher:
    """cORBmatcher(nnratio, checkOri, featDim, havingMasks) (src/cORBmatcher.cpp:46-65); brute-force searches only."""

    HISTO_LENGTH = 30

    def __init__(self, nnratio=0.6, checkOri=True, featDim=32, havingMasks_=False, ctx=None, K=8):
        self.mfNNratio, self.mbCheckOrientation, self.mbFeatDim, self.havingMasks = nnratio, checkOri, featDim, havingMasks_
        if havingMasks_:
            self.TH_HIGH_, self.TH_LOW_ = int(np.floor(1.5 * featDim)), int(np.floor(featDim))
        else:
            self.TH_HIGH_, self.TH_LOW_ = 3 * featDim, 2 * featDim
        self.ctx = ctx or default_context()
        self.K = K
        self.last_fallbacks = 0

    def _rot_filter(self, variant, keys_slot, keys_partner, match, swapped, accepted=None):
        """mbCheckOrientation: rotation-consistency filter (mcs_rotation_consistency) on `match` (slot -> partner index or -1), in place.
        -> number of matches removed (0 when the matcher was built with checkOri = False)."""
        if not self.mbCheckOrientation or len(match) == 0:
            return 0
        ks, kp = np.ascontiguousarray(keys_slot), np.ascontiguousarray(keys_partner)
        if len(kp) == 0:
            return 0
        off = KP_DTYPE.fields["angle"][1]
        acc = None if accepted is None else np.ascontiguousarray(accepted, np.int32)
        rem = np.zeros(1, np.int32)
        check(lib().mcs_rotation_consistency(self.ctx.h, variant, C.c_void_p(ks.ctypes.data + off), KP_DTYPE.itemsize, C.c_void_p(kp.ctypes.data + off),
                                             KP_DTYPE.itemsize, np_ptr(acc), np_ptr(match), len(match), len(kp), int(swapped), MEM_HOST, np_ptr(rem)))
        return int(rem[0])

    def _sets(self, d1, m1, v1, g1, d2, m2, v2, g2):
        keep = [np.ascontiguousarray(d1, np.uint8), np.ascontiguousarray(d2, np.uint8)]
        mm = [None, None]
        if self.havingMasks:
            mm = [np.ascontiguousarray(m1, np.uint8), np.ascontiguousarray(m2, np.uint8)]
        q = DescSet(np_ptr(keep[0]), np_ptr(mm[0]), np_ptr(v1), np_ptr(g1), keep[0].shape[0], self.mbFeatDim)
        t = DescSet(np_ptr(keep[1]), np_ptr(mm[1]), np_ptr(v2), np_ptr(g2), keep[1].shape[0], self.mbFeatDim)
        return q, t, (keep, mm, v1, v2, g1, g2)

    def SearchByBoW(self, pKF1, other):
        """(KF,KF) -> (nmatches, vpMatches12) with vpMatches12[idx1] = map point of KF2 (src/cORBmatcher.cpp:885-966);
        (KF,F)  -> (nmatches, vpMapPointMatches) indexed by frame feature (:179-323, vocabulary restriction removed)."""
        mp1 = pKF1.GetMapPointMatches()
        v1 = np.array([_good(m) for m in mp1], np.uint8)
        fb = np.zeros(1, np.int32)
        nm = np.zeros(1, np.int32)
        if isinstance(other, cMultiKeyFrame):
            mp2 = other.GetMapPointMatches()
            v2 = np.array([_good(m) for m in mp2], np.uint8)
            q, t, keep = self._sets(pKF1._d, pKF1._m, v1, None, other._d, other._m, v2, None)
            m12 = np.full(max(len(mp1), 1), -1, np.int32)
            check(lib().mcs_search_kf_kf(self.ctx.h, 1, C.byref(q), 0, C.byref(t), 0, self.mbFeatDim, self.mfNNratio, self.K, MEM_HOST,
                                         np_ptr(m12), np_ptr(nm), np_ptr(fb)))
            self.last_fallbacks = int(fb[0])
            return int(nm[0]), [mp2[j] if j >= 0 else None for j in m12[:len(mp1)]]
        F = other
        kfv, ffv = getattr(pKF1, "mFeatVec", None), getattr(F, "mFeatVec", None)
        if kfv and ffv:
            # the reference's vocabulary-restricted search: a keyframe feature only meets frame features of the same FeatureVector node;
            # nodes ascending, the features of a node in index order = keyframe rows permuted to (node, index) order, node id as `group`
            order = np.array([i for _, lst in kfv.items() for i in lst], np.int64)
            gk = np.array([nd for nd, lst in kfv.items() for _ in lst], np.int32)
            gf = np.full(F.totalN, -1, np.int32)
            for nd, lst in ffv.items():
                gf[lst] = nd
            vf = (gf >= 0).astype(np.uint8)
            q, t, keep = self._sets(pKF1._d[order], pKF1._m[order], np.ascontiguousarray(v1[order]), gk, F.all_descriptors(), F.all_masks(), vf, gf)
            mF = np.full(max(F.totalN, 1), -1, np.int32)
            check(lib().mcs_search_kf_f(self.ctx.h, 1, C.byref(q), 0, C.byref(t), 0, self.mbFeatDim, self.mfNNratio, self.K, MEM_HOST, np_ptr(mF),
                                        np_ptr(nm), np_ptr(fb)))
            self.last_fallbacks = int(fb[0])
            mF = np.where(mF[:F.totalN] >= 0, order[np.maximum(mF[:F.totalN], 0)], -1).astype(np.int32)   # back to keyframe feature indices
            removed = self._rot_filter(0, F.mvKeys, pKF1.mvKeys, mF, True)
            return int(nm[0]) - removed, [mp1[int(i)] if i >= 0 else None for i in mF]
        q, t, keep = self._sets(pKF1._d, pKF1._m, v1, None, F.all_descriptors(), F.all_masks(), None, None)
        mF = np.full(max(F.totalN, 1), -1, np.int32)
        check(lib().mcs_search_kf_f(self.ctx.h, 1, C.byref(q), 0, C.byref(t), 0, self.mbFeatDim, self.mfNNratio, self.K, MEM_HOST, np_ptr(mF),
                                    np_ptr(nm), np_ptr(fb)))
        self.last_fallbacks = int(fb[0])
        mF = np.ascontiguousarray(mF[:F.totalN])
        removed = self._rot_filter(0, F.mvKeys, pKF1.mvKeys, mF, True)
        return int(nm[0]) - removed, [mp1[i] if i >= 0 else None for i in mF]

    def SearchByProjection(self, F, vpMapPoints, th, *rest):
        """int SearchByProjection(cMultiFrame &F, const vector<cMapPoint*> &vpMapPoints, const double th) (src/cORBmatcher.cpp:67-166).
        Map points carry what isInFrustum() left on them (src/cMultiFrame.cpp:218-270): mbTrackInView[cam], mTrackProjX/Y[cam],
        mnTrackScaleLevel[cam], mTrackViewCos[cam], plus GetDescriptor()/GetDescriptorMask() (numpy rows).  Fills F.mvpMapPoints.
        The reference's other overloads dispatch on the argument types like C++ would: (CurrentFrame, LastFrame, th) -> SearchByProjectionLast,
        (F1, F2, windowSize, vpMapPointMatches2) -> SearchByProjectionFrames."""
        if isinstance(vpMapPoints, cMultiFrame):
            if rest:
                return self.SearchByProjectionFrames(F, vpMapPoints, th, rest[0])
            return self.SearchByProjectionLast(F, vpMapPoints, th)
        from ._capi import ProjectionSet
        nr = F.camSystem.GetNrCams()
        owner, px, py, vc, lv, pc, dd, mm = [], [], [], [], [], [], [], []
        for pMP in vpMapPoints:                       # the reference's visiting order: map point, then camera
            if pMP.isBad():
                continue
            for cam in range(nr):
                if not pMP.mbTrackInView[cam]:
                    continue
                owner.append(pMP); px.append(pMP.mTrackProjX[cam]); py.append(pMP.mTrackProjY[cam]); vc.append(pMP.mTrackViewCos[cam])
                lv.append(pMP.mnTrackScaleLevel[cam]); pc.append(cam); dd.append(pMP.GetDescriptor())
                if self.havingMasks:
                    mm.append(pMP.GetDescriptorMask())
        n = len(owner)
        if n == 0:
            return 0
        px, py, vc = (np.ascontiguousarray(v, np.float64) for v in (px, py, vc))
        lv, pc = np.ascontiguousarray(lv, np.int32), np.ascontiguousarray(pc, np.int32)
        dd = np.ascontiguousarray(np.stack(dd), np.uint8)
        mm = np.ascontiguousarray(np.stack(mm), np.uint8) if self.havingMasks else None
        mp = ProjectionSet(np_ptr(px), np_ptr(py), np_ptr(vc), np_ptr(lv), np_ptr(pc), np_ptr(dd), np_ptr(mm), n, self.mbFeatDim)
        fv, keep = _frame_view(F, self.mbFeatDim, self.havingMasks, np.array([m is not None for m in F.mvpMapPoints], np.uint8))
        match = np.full(n, -1, np.int32)
        nm = np.zeros(1, np.int32)
        check(lib().mcs_search_by_projection(self.ctx.h, C.byref(mp), C.byref(fv), float(th), self.mfNNratio, self.mbFeatDim, MEM_HOST, np_ptr(match),
                                             np_ptr(nm)))
        for p, j in enumerate(match):
            if j >= 0:
                F.mvpMapPoints[int(j)] = owner[p]
        return int(nm[0])

    # ------------------------------------------------------------------ grid-window searches other than (F, mapPoints)
    def _window_match(self, rule, x, y, r, lo, hi, cam, rows, F1, F2, assigned):
        """probes (window centre / radius / level range / camera / descriptor row of F1) against frame F2 -> (match per probe, nmatches)"""
        from ._capi import WindowProbes
        n = len(rows)
        if n == 0:
            return np.zeros(0, np.int32), 0
        x, y, r = (np.ascontiguousarray(v, np.float64) for v in (x, y, r))
        lo, hi, cam = (np.ascontiguousarray(v, np.int32) for v in (lo, hi, cam))
        rows = np.asarray(rows, np.int64)
        dd = np.ascontiguousarray(F1.all_descriptors()[rows], np.uint8)
        mm = np.ascontiguousarray(F1.all_masks()[rows], np.uint8) if self.havingMasks else None
        self.last_accepted = np.full(n, -1, np.int32)
        pr = WindowProbes(np_ptr(x), np_ptr(y), np_ptr(r), np_ptr(lo), np_ptr(hi), np_ptr(cam), np_ptr(dd), np_ptr(mm), n, self.mbFeatDim,
                          np_ptr(self.last_accepted) if rule == 3 else None)
        fv, keep = _frame_view(F2, self.mbFeatDim, self.havingMasks, assigned)
        match = np.full(n, -1, np.int32)
        nm = np.zeros(1, np.int32)
        check(lib().mcs_window_match(self.ctx.h, C.byref(pr), C.byref(fv), rule, self.mfNNratio, self.mbFeatDim, MEM_HOST, np_ptr(match), np_ptr(nm)))
        return match, int(nm[0])

    def BestInWindows(self, x, y, r, lo, hi, cam, desc, mask, F, max_dist, skip_taken=False, assigned=None):
        """The search loop of Fuse (src/cORBmatcher.cpp:1265-1719), SearchBySim3 (:1721-1988), SearchForTriangulationBetweenCameras (:1158-1263),
        SearchByProjection(pKF, Scw, ...) (:2265-2392) [skip_taken False] and of the relocalisation SearchByProjection(CurrentFrame, pKF,
        sAlreadyFound, th, ORBdist) (:2120-2263) [skip_taken True, `assigned` updated in place]: per probe (window centre x/y, radius r, level
        range lo..hi, camera, descriptor row) the closest feature of frame F inside the window -> (match [-1 if > max_dist], dist, nmatches)."""
        from ._capi import WindowProbes
        n = len(x)
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), 0
        x, y, r = (np.ascontiguousarray(v, np.float64) for v in (x, y, r))
        lo, hi, cam = (np.ascontiguousarray(v, np.int32) for v in (lo, hi, cam))
        dd = np.ascontiguousarray(desc, np.uint8)
        mm = np.ascontiguousarray(mask, np.uint8) if self.havingMasks else None
        pr = WindowProbes(np_ptr(x), np_ptr(y), np_ptr(r), np_ptr(lo), np_ptr(hi), np_ptr(cam), np_ptr(dd), np_ptr(mm), n, self.mbFeatDim)
        if skip_taken and assigned is None:
            assigned = np.array([m is not None for m in F.mvpMapPoints] + [0] * (F.totalN == 0), np.uint8)
        fv, keep = _frame_view(F, self.mbFeatDim, self.havingMasks, assigned if skip_taken else None)
        match, dist, nm = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(1, np.int32)
        check(lib().mcs_window_best(self.ctx.h, C.byref(pr), C.byref(fv), int(max_dist), int(bool(skip_taken)), self.mbFeatDim, MEM_HOST, np_ptr(match),
                                    np_ptr(dist), np_ptr(nm)))
        return match, dist, int(nm[0])

    def WindowSearch(self, F1, F2, windowSize, minScaleLevel=0, maxScaleLevel=2**31 - 1):
        """-> (nmatches, vpMapPointMatches2) (src/cORBmatcher.cpp:326-473)."""
        from ._capi import WINDOW_RATIO
        rows = [i for i, mp in enumerate(F1.mvpMapPoints) if _good(mp) and not (minScaleLevel > 0 and F1.mvKeys[i]["octave"] < minScaleLevel)
                and not (maxScaleLevel < 2**31 - 1 and F1.mvKeys[i]["octave"] > maxScaleLevel)]
        k = F1.mvKeys[rows]
        n = len(rows)
        assigned = np.zeros(max(F2.totalN, 1), np.uint8)
        match, nm = self._window_match(WINDOW_RATIO, k["x"].astype(np.float64), k["y"].astype(np.float64), np.full(n, float(windowSize)), np.full(n, -1),
                                       np.full(n, -1), F1.keypoint_to_cam[rows], rows, F1, F2, assigned)
        self.last_matches21 = np.full(F2.totalN, -1, np.int32)
        for p, j in enumerate(match):
            if j >= 0:
                self.last_matches21[int(j)] = rows[p]
        nm -= self._rot_filter(1, F2.mvKeys, F1.mvKeys, self.last_matches21, True)
        out = [F1.mvpMapPoints[int(i)] if i >= 0 else None for i in self.last_matches21]
        return nm, out

    def SearchByProjectionFrames(self, F1, F2, windowSize, vpMapPointMatches2):
        """int SearchByProjection(F1, F2, windowSize, vpMapPointMatches2) (src/cORBmatcher.cpp:476-577); the list is filled in place."""
        from ._capi import WINDOW_RATIO
        vpMapPointMatches2[:] = list(F2.mvpMapPoints)
        found = set(id(m) for m in vpMapPointMatches2 if m is not None)
        nr = F1.camSystem.GetNrCams()
        seen, sel = set(), []
        for i1, mp in enumerate(F1.mvpMapPoints):
            if mp is None or (hasattr(mp, "isBad") and mp.isBad()) or id(mp) in found or id(mp) in seen:
                continue
            seen.add(id(mp))
            sel.append(i1)
        if not sel:
            return 0
        pts = np.repeat(np.stack([np.asarray(F1.mvpMapPoints[i].GetWorldPos(), np.float64)[:3] for i in sel]), nr, axis=0)
        cams = np.tile(np.arange(nr, dtype=np.int32), len(sel))
        uv, fl = F2.camSystem.world_to_cam(pts, cams, self.ctx)
        ok = (fl & 1) != 0
        rows = np.repeat(np.asarray(sel), nr)[ok]
        lv = F1.mvKeys["octave"][rows]
        n = len(rows)
        assigned = np.array([m is not None for m in vpMapPointMatches2] + [0] * (F2.totalN == 0), np.uint8)
        match, nm = self._window_match(WINDOW_RATIO, uv[ok, 0], uv[ok, 1], np.full(n, float(windowSize)), lv, lv, cams[ok], rows, F1, F2, assigned)
        for p, j in enumerate(match):
            if j >= 0:
                vpMapPointMatches2[int(j)] = F1.mvpMapPoints[int(rows[p])]
        return nm

    def SearchByProjectionLast(self, CurrentFrame, LastFrame, th):
        """int SearchByProjection(CurrentFrame, LastFrame, th) (src/cORBmatcher.cpp:1990-2118); fills CurrentFrame.mvpMapPoints."""
        from ._capi import WINDOW_BEST
        sel = [i for i, mp in enumerate(LastFrame.mvpMapPoints) if _good(mp) and not LastFrame.mvbOutlier[i]]
        if not sel:
            return 0
        pts = np.stack([np.asarray(LastFrame.mvpMapPoints[i].GetWorldPos(), np.float64)[:3] for i in sel])
        cams = np.ascontiguousarray(LastFrame.keypoint_to_cam[sel], np.int32)
        uv, fl = CurrentFrame.camSystem.world_to_cam(pts, cams, self.ctx)
        ok = (fl & 1) != 0
        rows = np.asarray(sel)[ok]
        octv = LastFrame.mvKeys["octave"][rows]
        radius = float(th) * np.asarray(CurrentFrame.mvScaleFactors, np.float64)[octv]
        assigned = np.array([m is not None for m in CurrentFrame.mvpMapPoints] + [0] * (CurrentFrame.totalN == 0), np.uint8)
        match, nm = self._window_match(WINDOW_BEST, uv[ok, 0], uv[ok, 1], radius, octv - 1, octv + 1, cams[ok], rows, LastFrame, CurrentFrame, assigned)
        mcur = np.full(CurrentFrame.totalN, -1, np.int32)
        for p, j in enumerate(match):
            if j >= 0:
                mcur[int(j)] = rows[p]
        nm -= self._rot_filter(0, CurrentFrame.mvKeys, LastFrame.mvKeys, mcur, True)
        for j, i in enumerate(mcur):
            if i >= 0:
                CurrentFrame.mvpMapPoints[j] = LastFrame.mvpMapPoints[int(i)]
        return nm

    def SearchForInitialization(self, F1, F2, vbPrevMatched, windowSize=10):
        """-> (nmatches, vnMatches12); vbPrevMatched ([n1,2] float64) is updated in place (src/cORBmatcher.cpp:579-726)."""
        from ._capi import WINDOW_INITIALIZE
        n = F1.totalN
        rows = np.arange(n)
        lv = F1.mvKeys["octave"].astype(np.int32)
        match, nm = self._window_match(WINDOW_INITIALIZE, vbPrevMatched[:, 0], vbPrevMatched[:, 1], np.full(n, float(windowSize)), lv, lv,
                                       F1.keypoint_to_cam, rows, F1, F2, None)
        nm -= self._rot_filter(2, F1.mvKeys, F2.mvKeys, match, False, self.last_accepted)
        for i1, j in enumerate(match):
            if j >= 0:
                vbPrevMatched[i1, 0], vbPrevMatched[i1, 1] = float(F2.mvKeys[int(j)]["x"]), float(F2.mvKeys[int(j)]["y"])
        return nm, match

    def SearchForTriangulationRaw(self, pKF1, pKF2, Es):
        """-> (nmatches, vMatchedKeys1, vMatchedKeysRays1, vMatchedKeys2, vMatchedKeysRays2, vMatchedPairs) (:968-1155).
        Es: [nrCams][nrCams] 3x3 essential matrices (the reference precomputes them from the rig poses, :990-1003)."""
        nr = pKF1.camSystem.GetNrCams()
        E = np.ascontiguousarray(np.asarray(Es, np.float64).reshape(nr * nr, 9))
        v1 = np.array([m is None for m in pKF1.GetMapPointMatches()], np.uint8)    # "if (pMP1) continue"
        v2 = np.array([m is None for m in pKF2.GetMapPointMatches()], np.uint8)
        g1 = np.ascontiguousarray(pKF1.keypoint_to_cam, np.int32)
        g2 = np.ascontiguousarray(pKF2.keypoint_to_cam, np.int32)
        q, t, keep = self._sets(pKF1._d, pKF1._m, v1, g1, pKF2._d, pKF2._m, v2, g2)
        r1 = np.ascontiguousarray(pKF1.mvKeysRays, np.float64)
        r2 = np.ascontiguousarray(pKF2.mvKeysRays, np.float64)
        m12 = np.full(max(len(v1), 1), -1, np.int32)
        nm = np.zeros(1, np.int32)
        fb = np.zeros(1, np.int32)
        check(lib().mcs_search_triangulation(self.ctx.h, 1, C.byref(q), 0, C.byref(t), 0, np_ptr(r1), np_ptr(r2), np_ptr(E), nr, self.mbFeatDim,
                                             max(self.K, 16), MEM_HOST, np_ptr(m12), np_ptr(nm), np_ptr(fb)))
        self.last_fallbacks = int(fb[0])
        m12 = np.ascontiguousarray(m12[:len(v1)])
        nm[0] -= self._rot_filter(3, pKF1.mvKeys, pKF2.mvKeys, m12, False)
        pairs = [(i, int(j)) for i, j in enumerate(m12) if j >= 0]
        i1 = [p[0] for p in pairs]
        i2 = [p[1] for p in pairs]
        return int(nm[0]), pKF1.mvKeys[i1], pKF1.mvKeysRays[i1], pKF2.mvKeys[i2], pKF2.mvKeysRays[i2], pairs


COS_THRESH = float(np.cos(3.0 * np.pi / 180.0))   # src/cLocalMapping.cpp:39
MAX_DIST = 25.0                                   # :43


def _kf_geom(pKF, with_mp):
    """mcs_kf_geom of a keyframe (host arrays) -> (struct, keepalive)"""
    from ._capi import KfGeom
    cs = pKF.camSystem
    nr = cs.GetNrCams()
    ocs = (type(cs.cams[0].ocam) * nr)(*[cm.ocam for cm in cs.cams])
    keep = [np.ascontiguousarray(np.stack(cs.MtMc).reshape(nr, 16)), np.ascontiguousarray(np.stack(cs.MtMc_inv).reshape(nr, 16)),
            np.ascontiguousarray(cs.M_t, np.float64), ocs, np.ascontiguousarray(pKF.mvKeysRays, np.float64).reshape(-1, 3),
            np.ascontiguousarray(pKF.mvKeys), np.ascontiguousarray(pKF.keypoint_to_cam, np.int32)]
    g = KfGeom()
    g.MtMc, g.MtMc_inv, g.M_t, g.cams = keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, C.addressof(ocs)
    g.rays, g.keys, g.cam, g.n, g.nr_cams = keep[4].ctypes.data, keep[5].ctypes.data, keep[6].ctypes.data, len(keep[5]), nr
    if with_mp:
        idx = [i for i, mp in enumerate(pKF.mvpMapPoints) if mp is not None]
        pos = np.ascontiguousarray(np.array([np.asarray(pKF.mvpMapPoints[i].GetWorldPos(), np.float64)[:3] for i in idx]).reshape(-1, 3))
        cam = np.ascontiguousarray(keep[6][idx], np.int32)
        keep += [pos, cam]
        g.mp_pos, g.mp_cam, g.n_mp = pos.ctypes.data, cam.ctypes.data, len(idx)
    return g, keep


def CreateNewMapPoints(pKF, vpNeighKFs, checkOrientation=False, featDim=32, havingMasks=False, cosThresh=COS_THRESH, maxDIST=MAX_DIST, ctx=None, K=16,
                       valid1=None):
    """cLocalMapping::CreateNewMapPoints (src/cLocalMapping.cpp:223-381) in ONE device call (mcs_create_new_map_points): the current keyframe against its
    neighbours in the given order (GetBestCovisibilityKeyFrames), every neighbour searched with the features that earlier neighbours gave a map point
    taken out.  -> (per neighbour dict(idx1, idx2, x3D: the accepted matches in the reference's order; verdict, x3D_all, match12, nmatches, fallbacks,
    baseline, medianDepth, skipped), final valid1).  Creating the cMapPoint objects (new cMapPoint, AddObservation, AddMapPoint, :362-377) stays with
    the caller; valid1 (default: "has no map point yet") lets a second call continue a neighbour list."""
    from ._capi import KfGeom, NewPointsOut
    ns = len(vpNeighKFs)
    if ns == 0:
        return [], np.array([m is None for m in pKF.mvpMapPoints], bool)
    ctx = ctx or default_context()
    g1, keep = _kf_geom(pKF, False)
    n1 = g1.n

    def dset(kf, g, valid):
        d = np.ascontiguousarray(kf._d, np.uint8)
        m = np.ascontiguousarray(kf._m, np.uint8) if havingMasks else None
        v = np.ascontiguousarray(valid, np.uint8)
        keep.extend([d, m, v])
        return DescSet(np_ptr(d), np_ptr(m), np_ptr(v), g.cam, len(d), featDim)

    s1 = dset(pKF, g1, [m is None for m in pKF.mvpMapPoints] if valid1 is None else valid1)
    g2, s2 = (KfGeom * ns)(), (DescSet * ns)()
    for s, kf in enumerate(vpNeighKFs):
        g, k = _kf_geom(kf, True)
        keep.append(k)
        g2[s], s2[s] = g, dset(kf, g, [m is None for m in kf.mvpMapPoints])
    rows = max(ns * n1, 1)
    verdict, x3D, cnt = np.zeros(rows, np.int32), np.zeros((rows, 3)), np.zeros(ns, np.int32)
    a1, a2, ax = np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros((rows, 3))
    out = NewPointsOut(np_ptr(verdict).value, np_ptr(x3D).value, np_ptr(cnt).value, np_ptr(a1).value, np_ptr(a2).value, np_ptr(ax).value)
    m12, nm, fb = np.full(rows, -1, np.int32), np.zeros(ns, np.int32), np.zeros(ns, np.int32)
    bl, md, sk, v1 = np.zeros(ns), np.zeros(ns), np.zeros(ns, np.uint8), np.zeros(max(n1, 1), np.uint8)
    check(lib().mcs_create_new_map_points(ctx.h, ns, C.byref(g1), C.byref(s1), g2, s2, None, 0, featDim, max(K, 16), int(bool(checkOrientation)),
                                          float(cosThresh), float(maxDIST), MEM_HOST, np_ptr(m12), np_ptr(nm), np_ptr(fb), np_ptr(bl), np_ptr(md), np_ptr(sk),
                                          np_ptr(v1), C.byref(out)))
    res = []
    for s in range(ns):
        k, lo = int(cnt[s]), s * n1
        res.append(dict(idx1=a1[lo:lo + k].copy(), idx2=a2[lo:lo + k].copy(), x3D=ax[lo:lo + k].copy(), verdict=verdict[lo:lo + n1].copy(),
                        x3D_all=x3D[lo:lo + n1].copy(), match12=m12[lo:lo + n1].copy(), nmatches=int(nm[s]), fallbacks=int(fb[s]), baseline=float(bl[s]),
                        medianDepth=float(md[s]), skipped=bool(sk[s])))
    return res, v1[:n1].astype(bool)


def _local_points(vpMapPoints, frame_id):
    """mcs_local_points of a list of map points (GetWorldPos, GetNormal, Get{Min,Max}DistanceInvariance, isBad, mnLastFrameSeen) + the arrays behind it"""
    from ._capi import LP_BAD, LP_SEEN, LocalPoints
    n = len(vpMapPoints)
    a = dict(pos=np.ascontiguousarray([np.asarray(m.GetWorldPos(), np.float64)[:3] for m in vpMapPoints], np.float64).reshape(n, 3),
             normal=np.ascontiguousarray([np.asarray(m.GetNormal(), np.float64)[:3] for m in vpMapPoints], np.float64).reshape(n, 3),
             min_dist=np.array([m.GetMinDistanceInvariance() for m in vpMapPoints], np.float64),
             max_dist=np.array([m.GetMaxDistanceInvariance() for m in vpMapPoints], np.float64),
             flags=np.array([(LP_BAD if m.isBad() else 0) | (LP_SEEN if frame_id is not None and getattr(m, "mnLastFrameSeen", None) == frame_id else 0)
                             for m in vpMapPoints], np.uint8))
    a["struct"] = LocalPoints(np_ptr(a["pos"]), np_ptr(a["normal"]), np_ptr(a["min_dist"]), np_ptr(a["max_dist"]), np_ptr(a["flags"]), n)
    return a


def _rig_arrays(camSystem, cams=None):
    """mcs_rig_view of a cMultiCamSys_ (all cameras, or the listed ones) + the arrays behind it"""
    from ._capi import RigView
    cams = list(range(camSystem.GetNrCams())) if cams is None else list(cams)
    nr = len(cams)
    a = dict(MtMc_inv=np.ascontiguousarray(np.stack([camSystem.MtMc_inv[c] for c in cams]).reshape(nr, 16)),
             MtMc=np.ascontiguousarray(np.stack([camSystem.MtMc[c] for c in cams]).reshape(nr, 16)))
    a["ocs"] = (type(camSystem.cams[0].ocam) * nr)(*[camSystem.cams[c].ocam for c in cams])
    masks = [camSystem.cams[c].GetMirrorMask(0) for c in cams]
    a["masks"] = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in masks]
    a["mp"] = (C.c_void_p * nr)(*[None if m is None else m.ctypes.data for m in a["masks"]])
    has = all(m is not None for m in a["masks"])
    a["struct"] = RigView(np_ptr(a["MtMc_inv"]), np_ptr(a["MtMc"]), C.cast(a["ocs"], C.c_void_p), C.cast(a["mp"], C.c_void_p) if has else None, nr)
    return a


class _Mem:
    """where the arrays of a call live, host memory (numpy arrays) or device memory (DeviceArray copies): put / ptr / read of an array and the MEM_* kind"""

    def __init__(self, device):
        self.device, self.kind = device, MEM_DEVICE if device else MEM_HOST
        self.put = lambda a: None if a is None else DeviceArray(a) if device else np.ascontiguousarray(a)
        self.ptr = lambda a: None if a is None else a.ptr if device else np_ptr(a)
        self.read = lambda a: a.read() if device else a


_HOST, _DEVICE = _Mem(False), _Mem(True)


def _frame_view(F, featDim, havingMasks, assigned, mem=_HOST):
    """mcs_frame_view of a cMultiFrame in host or device memory -> (FrameView, the arrays behind it by name); `assigned` is the host call's array itself"""
    from ._capi import FrameView
    a = dict(keys=F.mvKeys, desc=np.asarray(F.all_descriptors(), np.uint8), mask=np.asarray(F.all_masks(), np.uint8) if havingMasks else None,
             cam=np.asarray(F.keypoint_to_cam, np.int32), assigned=assigned, w=np.asarray(F.mnMaxX, np.int32), h=np.asarray(F.mnMaxY, np.int32),
             sc=np.asarray(F.mvScaleFactors, np.float64))
    a = {k: mem.put(v) for k, v in a.items()}
    fv = FrameView(*[mem.ptr(a[k]) for k in ("keys", "desc", "mask", "cam", "assigned")], F.totalN, featDim, F.camSystem.GetNrCams(), mem.ptr(a["w"]),
                   mem.ptr(a["h"]), mem.ptr(a["sc"]), len(F.mvScaleFactors))
    return fv, a


def _rig_view(camSystem, mem=_HOST, cams=None):
    """mcs_rig_view of a cMultiCamSys_ (all cameras, or the listed ones) in host or device memory -> (RigView, keepalive)"""
    from ._capi import RigView
    rig = _rig_arrays(camSystem, cams)
    if not mem.device:
        return rig["struct"], rig
    keep = [DeviceArray(rig["MtMc_inv"]), DeviceArray(rig["MtMc"]), DeviceArray(np.frombuffer(rig["ocs"], np.uint8).copy())]
    mp = None
    if all(m is not None for m in rig["masks"]):
        md = [DeviceArray(m) for m in rig["masks"]]
        mp = DeviceArray(np.array([m.ptr.value for m in md], np.uint64))
        keep += md + [mp]
    return RigView(keep[0].ptr, keep[1].ptr, keep[2].ptr, mp.ptr if mp else None, len(rig["masks"])), keep


def SearchReferencePointsInFrustum(F, vpLocalMapPoints, th=3, nnratio=0.8, featDim=32, havingMasks=False, ctx=None):
    """int cTracking::SearchReferencePointsInFrustum() (src/cTracking.cpp:953-1012) for frame F (mCurrentFrame) and vpLocalMapPoints (mvpLocalMapPoints).
    The first loop (:957-976) runs here as written; isInFrustum for every local point in every camera, the nToMatch gate and
    cORBmatcher(nnratio).SearchByProjection(F, vpLocalMapPoints, th) are ONE device call (mcs_search_local_points).  The tracking fields and
    IncreaseVisible() counts are written back onto the map points, F.mvpMapPoints is filled, the reference's value is returned.  Map points:
    GetWorldPos(), GetNormal(), GetMinDistanceInvariance(), GetMaxDistanceInvariance(), isBad(), IncreaseVisible(), mnLastFrameSeen, GetDescriptor() /
    GetDescriptorMask() (numpy rows) and the per-camera lists mbTrackInView, mTrackProjX, mTrackProjY, mnTrackScaleLevel, mTrackViewCos."""
    from ._capi import TrackState
    ctx = ctx or default_context()
    nr = F.camSystem.GetNrCams()
    nrMatches = 0
    for i, pMP in enumerate(F.mvpMapPoints):     # :957-976
        if pMP is None:
            continue
        if pMP.isBad():
            F.mvpMapPoints[i] = None
            continue
        pMP.IncreaseVisible()
        pMP.mnLastFrameSeen = F.mnId
        pMP.mbTrackInView[int(F.keypoint_to_cam[i])] = False
        nrMatches += 1
    n = len(vpLocalMapPoints)
    if n == 0:
        return nrMatches
    pts = _local_points(vpLocalMapPoints, F.mnId)
    rv, keep = _rig_view(F.camSystem)
    st = dict(in_view=np.array([[bool(v) for v in m.mbTrackInView[:nr]] for m in vpLocalMapPoints], np.uint8),
              proj_x=np.array([m.mTrackProjX[:nr] for m in vpLocalMapPoints], np.float64), proj_y=np.array([m.mTrackProjY[:nr] for m in vpLocalMapPoints], np.float64),
              level=np.array([m.mnTrackScaleLevel[:nr] for m in vpLocalMapPoints], np.int32), view_cos=np.array([m.mTrackViewCos[:nr] for m in vpLocalMapPoints], np.float64))
    ts = TrackState(*[np_ptr(st[k]) for k in ("in_view", "proj_x", "proj_y", "level", "view_cos")])
    dd = np.ascontiguousarray(np.stack([m.GetDescriptor() for m in vpLocalMapPoints]), np.uint8)
    mm = np.ascontiguousarray(np.stack([m.GetDescriptorMask() for m in vpLocalMapPoints]), np.uint8) if havingMasks else None
    fv, fa = _frame_view(F, featDim, havingMasks, np.array([m is not None for m in F.mvpMapPoints] or [0], np.uint8))
    match, vis = np.full(n * nr, -1, np.int32), np.zeros(n, np.int32)
    nm, ntm = np.zeros(1, np.int32), np.zeros(1, np.int32)
    check(lib().mcs_search_local_points(ctx.h, C.byref(pts["struct"]), C.byref(rv), C.byref(ts), np_ptr(dd), np_ptr(mm), featDim, C.byref(fv), float(th),
                                        float(nnratio), featDim, MEM_HOST, np_ptr(match), np_ptr(nm), np_ptr(ntm), np_ptr(vis)))
    for i, pMP in enumerate(vpLocalMapPoints):
        for _ in range(int(vis[i])):             # :995
            pMP.IncreaseVisible()
        if pts["flags"][i]:                      # the loop :981-999 never touched this point
            continue
        for c in range(nr):
            pMP.mbTrackInView[c] = bool(st["in_view"][i, c])
            pMP.mTrackProjX[c], pMP.mTrackProjY[c] = float(st["proj_x"][i, c]), float(st["proj_y"][i, c])
            pMP.mnTrackScaleLevel[c], pMP.mTrackViewCos[c] = int(st["level"][i, c]), float(st["view_cos"][i, c])
    for p in np.flatnonzero(match >= 0):
        F.mvpMapPoints[int(match[p])] = vpLocalMapPoints[int(p) // nr]     # F.mvpMapPoints[bestIdx] = pMP, src/cORBmatcher.cpp:159
    SearchReferencePointsInFrustum.last = dict(nToMatch=int(ntm[0]), nmatches=int(nm[0]), match=match.reshape(n, nr))
    return nrMatches + int(nm[0])


def DescriptorDistance64(descr_i, descr_j, dim=32, ctx=None):
    return (ctx or default_context()).descriptor_distance(np.frombuffer(descr_i, np.uint8)[:dim], np.frombuffer(descr_j, np.uint8)[:dim])


def DescriptorDistance64Masked(descr_i, descr_j, mask_i, mask_j, dim=32, ctx=None):
    f = lambda a: np.frombuffer(a, np.uint8)[:dim]
    return (ctx or default_context()).descriptor_distance(f(descr_i), f(descr_j), f(mask_i), f(mask_j))


def ComputeDistinctiveDescriptorsBatch(observed, dim=32, ctx=None):
    """cMapPoint::ComputeDistinctiveDescriptors (src/cMapPoint.cpp:294-382) for many map points in one device call.
    observed: one (descriptors [N_k, dim] uint8, masks [N_k, dim] uint8 or None) pair per map point, rows in the order the reference's loop
    collects them.  -> int32 array, the chosen row per map point (-1 where N_k == 0: the reference keeps the old descriptor)."""
    n = len(observed)
    if n == 0:
        return np.zeros(0, np.int32)
    having = observed[0][1] is not None
    counts = [len(d) for d, _ in observed]
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum(counts)
    rows = int(off[-1])
    dd = np.zeros((max(rows, 1), dim), np.uint8)
    mm = np.zeros((max(rows, 1), dim), np.uint8) if having else None
    for k, (d, m) in enumerate(observed):
        if counts[k]:
            dd[off[k]:off[k + 1]] = d
            if having:
                mm[off[k]:off[k + 1]] = m
    best = np.full(n, -1, np.int32)
    ctx = ctx or default_context()
    check(lib().mcs_distinctive_descriptors(ctx.h, np_ptr(dd), np_ptr(mm), dim, dim, np_ptr(off), n, MEM_HOST, np_ptr(best)))
    return best


class cMapPoint:
    """The descriptor side of cMapPoint (include/cMapPoint.h): observations -> representative descriptor (+ mask)."""

    def __init__(self, Pos=None, ctx=None):
        self.mWorldPos = None if Pos is None else np.asarray(Pos, np.float64)
        self.mObservations = []          # [(keyframe, [feature indices])] in insertion order (the reference's std::map orders by POINTER)
        self.mDescriptor = self.mDescriptorMask = None
        self.mbBad = False
        self.ctx = ctx

    def isBad(self):
        return self.mbBad

    def GetWorldPos(self):
        return self.mWorldPos

    def AddObservation(self, pKF, idx):
        for kf, lst in self.mObservations:
            if kf is pKF:
                lst.append(int(idx))
                return
        self.mObservations.append((pKF, [int(idx)]))

    def GetIndexInKeyFrame(self, pKF):
        """the feature indices of this point in pKF (empty if it has no observation there)"""
        for kf, lst in self.mObservations:
            if kf is pKF:
                return list(lst)
        return []

    def _observed(self, havingMasks):
        d, m = [], []
        for kf, lst in self.mObservations:
            if hasattr(kf, "isBad") and kf.isBad():
                continue
            for l in lst:
                d.append(kf._d[l])
                if havingMasks:
                    m.append(kf._m[l])
        dim = d[0].shape[0] if d else 32
        return (np.stack(d) if d else np.zeros((0, dim), np.uint8)), ((np.stack(m) if m else np.zeros((0, dim), np.uint8)) if havingMasks else None)

    def ComputeDistinctiveDescriptors(self, havingMasks):
        if self.mbBad or not self.mObservations:
            return
        d, m = self._observed(havingMasks)
        if len(d) == 0:
            return
        b = int(ComputeDistinctiveDescriptorsBatch([(d, m)], d.shape[1], self.ctx)[0])
        self.mDescriptor = d[b].copy()
        if havingMasks:
            self.mDescriptorMask = m[b].copy()

    def GetDescriptor(self):
        return self.mDescriptor

    def GetDescriptorMask(self):
        return self.mDescriptorMask


class cORBVocabulary:
    """ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (include/cORBVocabulary.h) as far as the front end uses it:
    transform(features, levelsup) -> (BowVector, FeatureVector) (ThirdParty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1205).  The tree descent of
    every descriptor runs on the GPU (mcs_bow_transform); the two std::map's are rebuilt here with the reference's arithmetic order."""

    def __init__(self, voc, ctx=None):
        """voc: the dict of multicol-slam_amd.io.load_vocabulary (or a path to the vocabulary YAML)."""
        if isinstance(voc, str):
            from . import io as _io
            voc = _io.load_vocabulary(voc)
        self.voc = voc
        self.ctx = ctx or default_context()
        self.m_k, self.m_L = voc["k"], voc["L"]
        if voc["scoringType"] != 0 or voc["weightingType"] != 0:
            raise NotImplementedError("only TF_IDF weighting with L1 scoring (the shipped small_orb_omni_voc_9_6.yml) is mirrored")
        self.h = C.c_void_p()
        nd = np.ascontiguousarray(voc["node_desc"], np.uint8)
        co, ci = np.ascontiguousarray(voc["child_off"], np.int32), np.ascontiguousarray(voc["child_idx"], np.int32)
        check(lib().mcs_vocabulary_create(self.ctx.h, len(nd), np_ptr(nd), np_ptr(co), np_ptr(ci), self.m_L, C.byref(self.h)))
        wid, wt = np.ascontiguousarray(voc["word_id"], np.int32), np.ascontiguousarray(voc["weight"], np.float64)
        check(lib().mcs_vocabulary_set_words(self.h, np_ptr(wid), np_ptr(wt)))
        self.n_words = int(voc.get("n_words", int(wid.max()) + 1))

    def size(self):
        return self.n_words

    def __del__(self):
        try:
            if self.h:
                lib().mcs_vocabulary_destroy(self.h)
        except Exception:
            pass

    def descend(self, descriptors, levelsup):
        """-> (leaf node, node at level L - levelsup) per descriptor row"""
        d = np.ascontiguousarray(descriptors, np.uint8)
        n = len(d)
        leaf, nid = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        if n:
            check(lib().mcs_bow_transform(self.h, np_ptr(d), n, d.shape[1], int(levelsup), MEM_HOST, np_ptr(leaf), np_ptr(nid)))
        return leaf[:n], nid[:n]

    def transform(self, descriptors, levelsup=4):
        """-> (BowVector {word id: value}, FeatureVector {node id: [feature indices]}), both in ascending key order like std::map."""
        leaf, nid = self.descend(descriptors, levelsup)
        words, weights = self.voc["word_id"][leaf], self.voc["weight"][leaf]
        bow, fv = {}, {}
        for i in range(len(leaf)):            # TF_IDF branch: addWeight accumulates in feature order (:1147-1163)
            w = float(weights[i])
            if w > 0:
                wid = int(words[i])
                bow[wid] = bow.get(wid, 0.0) + w
                fv.setdefault(int(nid[i]), []).append(i)
        bow = dict(sorted(bow.items()))
        norm = 0.0                            # L1 scoring: mustNormalize -> BowVector::normalize(L1) in key order (BowVector.cpp)
        for v in bow.values():
            norm += abs(v)
        if norm > 0.0:
            bow = {k: v / norm for k, v in bow.items()}
        return bow, dict(sorted(fv.items()))

    def bow_vector(self, descriptors, levelsup=4):
        """The BowVector of transform() built on the device (mcs_bow_vector): -> (word ids int32 ascending, values float64), bit-identical to
        transform()'s dict."""
        leaf, _ = self.descend(descriptors, levelsup)
        n = len(leaf)
        w, v, nw = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float64), np.zeros(1, np.int32)
        check(lib().mcs_bow_vector(self.h, np_ptr(np.ascontiguousarray(leaf, np.int32)), n, MEM_HOST, np_ptr(w), np_ptr(v), np_ptr(nw)))
        return w[:nw[0]].copy(), v[:nw[0]].copy()

    def bow_vector_device(self, leaf_nodes_dev, n, word_ids_dev, values_dev, nwords_dev):
        """Device pointers (ints, e.g. torch tensor data_ptr()): leaf nodes of mcs_bow_transform -> BowVector, never leaving the GPU."""
        check(lib().mcs_bow_vector(self.h, C.c_void_p(leaf_nodes_dev), int(n), MEM_DEVICE, C.c_void_p(word_ids_dev), C.c_void_p(values_dev),
                                   C.c_void_p(nwords_dev)))


def _bow_arrays(bow):
    """mBowVec as a dict {word: value} (cORBVocabulary.transform) or a (word ids, values) pair (bow_vector) -> contiguous arrays"""
    if isinstance(bow, dict):
        items = sorted(bow.items())
        return np.array([k for k, _ in items], np.int32), np.array([v for _, v in items], np.float64)
    w, v = bow
    return np.ascontiguousarray(w, np.int32), np.ascontiguousarray(v, np.float64)


def _csr(bows):
    arrs = [_bow_arrays(b) for b in bows]
    off = np.zeros(len(arrs) + 1, np.int32)
    off[1:] = np.cumsum([len(w) for w, _ in arrs])
    w = np.concatenate([a[0] for a in arrs]) if arrs else np.zeros(0, np.int32)
    v = np.concatenate([a[1] for a in arrs]) if arrs else np.zeros(0, np.float64)
    return off, np.ascontiguousarray(w, np.int32), np.ascontiguousarray(v, np.float64)


class cMultiKeyFrameDatabase:
    """cMultiKeyFrameDatabase (include/cMultiKeyFrameDatabase.h, src/cMultiKeyFrameDatabase.cpp) on the device (mcs_kfdb_*).
    Keyframes need mnId and mBowVec; their covisibility (GetBestCovisibilityKeyFrames(10)) is read when they are added and whenever
    SetCovisibility / UpdateCovisibility is called.  Candidates come back as the keyframe objects that were added (or named as neighbours)."""

    def __init__(self, voc, ctx=None, capacity_hint=0):
        """voc: a cORBVocabulary (its word count sizes the inverted file, as mpVoc->size() does) or a word count."""
        n_words = voc.size() if hasattr(voc, "size") else int(voc)
        self.ctx = ctx or getattr(voc, "ctx", None) or default_context()
        self.mpVoc = voc
        self.h = C.c_void_p()
        check(lib().mcs_kfdb_create(self.ctx.h, int(n_words), int(capacity_hint), C.byref(self.h)))
        self.objects = {}   # mnId -> keyframe object
        self.diag_cap = 0   # > 0: the last query's diagnostics in self.last_trace (lists of (kf id, words, score, acc, best id))
        self.last_trace = None

    def __del__(self):
        try:
            if self.h:
                lib().mcs_kfdb_destroy(self.h)
        except Exception:
            pass

    def add(self, pKF):
        off, w, v = _csr([pKF.mBowVec])
        ids = np.array([pKF.mnId], np.int64)
        check(lib().mcs_kfdb_add(self.h, 1, np_ptr(ids), np_ptr(off), np_ptr(w), np_ptr(v), MEM_HOST))
        self.objects[int(pKF.mnId)] = pKF
        if hasattr(pKF, "GetBestCovisibilityKeyFrames"):
            self.SetCovisibility(pKF, pKF.GetBestCovisibilityKeyFrames(10))

    def erase(self, pKF):
        ids = np.array([pKF.mnId], np.int64)
        check(lib().mcs_kfdb_erase(self.h, 1, np_ptr(ids)))

    def clear(self):
        check(lib().mcs_kfdb_clear(self.h))

    def size(self):
        n = C.c_int32()
        check(lib().mcs_kfdb_size(self.h, C.byref(n)))
        return n.value

    def SetCovisibility(self, pKF, ordered_neighbours):
        nb = list(ordered_neighbours)[:10]
        for k in nb:
            self.objects.setdefault(int(k.mnId), k)
        ids = np.array([pKF.mnId], np.int64)
        arr = np.zeros(10, np.int64)
        arr[:len(nb)] = [k.mnId for k in nb]
        self.objects.setdefault(int(pKF.mnId), pKF)
        cnt = np.array([len(nb)], np.int32)
        check(lib().mcs_kfdb_set_covisibility(self.h, 1, np_ptr(ids), np_ptr(arr), np_ptr(cnt)))

    def UpdateCovisibility(self, kfs=None):
        for kf in (kfs if kfs is not None else list(self.objects.values())):
            if hasattr(kf, "GetBestCovisibilityKeyFrames"):
                self.SetCovisibility(kf, kf.GetBestCovisibilityKeyFrames(10))

    def _run(self, loop, ids, bows, connected=None, min_scores=None):
        nq = len(ids)
        off, w, v = _csr(bows)
        qid = np.ascontiguousarray(ids, np.int64)
        cap = max(16, 2 * len(self.objects))
        while True:
            cnt = np.zeros(max(nq, 1), np.int32)
            out = np.zeros(max(nq * cap, 1), np.int64)
            diag, dd = None, None
            if self.diag_cap > 0:
                dc = self.diag_cap
                dd = dict(count=np.zeros(max(nq, 1), np.int32), kf_id=np.zeros(nq * dc, np.int64), words=np.zeros(nq * dc, np.int32),
                          score=np.zeros(nq * dc), acc=np.zeros(nq * dc), best=np.zeros(nq * dc, np.int64))
                diag = KfdbDiag(dc, *[np_ptr(dd[k]) for k in ("count", "kf_id", "words", "score", "acc", "best")])
            if loop:
                coff = np.zeros(nq + 1, np.int32)
                coff[1:] = np.cumsum([len(c) for c in connected])
                cids = np.array([int(k.mnId) for c in connected for k in c], np.int64)
                ms = np.ascontiguousarray(min_scores, np.float64)
                rc = lib().mcs_kfdb_detect_loop(self.h, nq, np_ptr(qid), np_ptr(off), np_ptr(w), np_ptr(v), np_ptr(coff), np_ptr(cids) if len(cids) else None,
                                                np_ptr(ms), MEM_HOST, cap, np_ptr(cnt), np_ptr(out), C.byref(diag) if diag else None)
            else:
                rc = lib().mcs_kfdb_detect_relocalisation(self.h, nq, np_ptr(qid), np_ptr(off), np_ptr(w), np_ptr(v), MEM_HOST, cap, np_ptr(cnt), np_ptr(out),
                                                          C.byref(diag) if diag else None)
            if rc == MCS_ERR_CAPACITY and int(cnt[:nq].max(initial=0)) > cap:   # the state is unchanged: run again with room
                cap = int(cnt[:nq].max())
                continue
            check(rc)
            break
        if dd is not None:
            self.last_trace = [[(int(dd["kf_id"][q * dc + i]), int(dd["words"][q * dc + i]), float(dd["score"][q * dc + i]), float(dd["acc"][q * dc + i]),
                                 int(dd["best"][q * dc + i])) for i in range(int(dd["count"][q]))] for q in range(nq)]
        return [[self.objects[int(i)] for i in out[q * cap:q * cap + cnt[q]]] for q in range(nq)]

    def DetectRelocalisationCandidates(self, F):
        return self._run(False, [F.mnId], [F.mBowVec])[0]

    def detect_relocalisation(self, frames):
        """DetectRelocalisationCandidates of every frame, in one device call (= the calls one after another)."""
        return self._run(False, [F.mnId for F in frames], [F.mBowVec for F in frames]) if frames else []

    def DetectLoopCandidates(self, pKF, minScore, connected=None):
        """connected: pKF->GetConnectedKeyFrames() (default: pKF.GetConnectedKeyFrames() if it exists, else none)"""
        if connected is None:
            connected = pKF.GetConnectedKeyFrames() if hasattr(pKF, "GetConnectedKeyFrames") else []
        return self._run(True, [pKF.mnId], [pKF.mBowVec], [list(connected)], [float(minScore)])[0]

    def detect_loop(self, kfs, min_scores, connected):
        return self._run(True, [k.mnId for k in kfs], [k.mBowVec for k in kfs], [list(c) for c in connected], min_scores) if kfs else []

    def score(self, bow, kfs):
        """ORBVocabulary::score(bow, pKFi->mBowVec) for stored keyframes (src/cLoopClosing.cpp:132-151)"""
        w, v = _bow_arrays(bow)
        ids = np.array([k.mnId for k in kfs], np.int64)
        out = np.zeros(max(len(ids), 1))
        check(lib().mcs_kfdb_score(self.h, len(w), np_ptr(w), np_ptr(v), len(ids), np_ptr(ids), MEM_HOST, np_ptr(out)))
        return out[:len(ids)]


class cSim3SolverBatch:
    """Many cSim3Solver in one device batch (mcs_sim3_*): one iterate() call is one round of cLoopClosing::ComputeSim3 over all its candidates
    (src/cLoopClosing.cpp:304-330), which equals the reference's sequential round because the solvers are independent.  The solvers' state
    lives in the batch from here on; solver k draws as solver index k of `seed`."""

    def __init__(self, solvers, ctx=None, seed=None, draws=None):
        """solvers: cSim3Solver objects sharing one local rig; draws (optional): per solver an int array [max(1, maxIterations)][3] of randi."""
        self.solvers = list(solvers)
        s0 = self.solvers[0]
        self.ctx = ctx or s0.ctx
        self.seed = int(s0.seed if seed is None else seed)
        cs = s0.camSysLocal
        nr = cs.GetNrCams()
        ns = len(self.solvers)
        M_c = np.ascontiguousarray(np.stack([np.asarray(m, np.float64) for m in cs.M_c]).reshape(nr, 16))
        ocs = (type(cs.cams[0].ocam) * nr)(*[cm.ocam for cm in cs.cams])
        off = np.zeros(ns + 1, np.int32)
        off[1:] = np.cumsum([s.N for s in self.solvers])
        cat = lambda name, shape, dt: np.ascontiguousarray(np.concatenate([getattr(s, name) for s in self.solvers]).reshape(shape), dt) if off[-1] else np.zeros(shape, dt)
        nc = int(off[-1])
        self._n1 = np.array([s.mN1 for s in self.solvers], np.int32)
        Xw, cam, sig, idx = cat("_Xw", (nc, 2, 3), np.float64), cat("_cam", (nc, 2), np.int32), cat("_sig", (nc, 2), np.float64), cat("_idx1", (nc,), np.int32)
        Mt = np.ascontiguousarray(np.stack([s._Mt for s in self.solvers]), np.float64)
        MtMc = np.ascontiguousarray(np.stack([s._MtMc for s in self.solvers]), np.float64)
        p, mi, mx = self._params()
        dr = None
        if draws is not None:
            dr = np.ascontiguousarray(np.concatenate([np.asarray(d, np.int32).reshape(-1) for d in draws]), np.int32)
        self.h = C.c_void_p()
        check(lib().mcs_sim3_create(self.ctx.h, nr, np_ptr(M_c), ocs, ns, np_ptr(self._n1), np_ptr(off), np_ptr(Mt), np_ptr(MtMc), np_ptr(p), np_ptr(mi),
                                    np_ptr(mx), np_ptr(Xw), np_ptr(cam), np_ptr(sig), np_ptr(idx), C.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF),
                                    np_ptr(dr), C.byref(self.h)))
        self._keep = (Xw, cam, sig, idx, dr)
        for k, s in enumerate(self.solvers):
            s._batch, s._slot = self, k

    def _params(self):
        return (np.array([s.mRansacProb for s in self.solvers], np.float64), np.array([s.mRansacMinInliers for s in self.solvers], np.int32),
                np.array([s.mRansacMaxItsParam for s in self.solvers], np.int32))

    def __del__(self):
        try:
            if self.h:
                lib().mcs_sim3_destroy(self.h)
        except Exception:
            pass

    def SetRansacParameters(self):
        """push every solver's (probability, minInliers, maxIterations) to the device: mnIterations = 0, the best-so-far state stays"""
        p, mi, mx = self._params()
        check(lib().mcs_sim3_set_ransac_parameters(self.h, np_ptr(p), np_ptr(mi), np_ptr(mx)))

    def iterate(self, n):
        """n: iterations per solver (an int for all, or a list; <= 0 leaves a solver alone) -> [(success, bNoMore, vbInliers, nInliers, T12)], T12 the
        4x4 result where success, else None (the reference leaves the caller's matrix as it was)"""
        ns = len(self.solvers)
        nit = np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int32), (ns,)), np.int32)
        succ, nomore, ninl = np.zeros(ns, np.uint8), np.zeros(ns, np.uint8), np.zeros(ns, np.int32)
        T = np.zeros((ns, 16))
        vb = np.zeros(max(int(self._n1.sum()), 1), np.uint8)
        check(lib().mcs_sim3_iterate(self.h, np_ptr(nit), np_ptr(succ), np_ptr(nomore), np_ptr(ninl), np_ptr(T), np_ptr(vb)))
        out, o = [], 0
        for k in range(ns):
            n1 = int(self._n1[k])
            out.append((bool(succ[k]), bool(nomore[k]), vb[o:o + n1].astype(bool), int(ninl[k]), T[k].reshape(4, 4).copy() if succ[k] else None))
            o += n1
        return out

    def best(self):
        """-> (R [ns,3,3], t [ns,3], s [ns], T12 [ns,4,4], mnBestInliers [ns], mnIterations [ns])"""
        ns = len(self.solvers)
        R, t, s, T = np.zeros((ns, 9)), np.zeros((ns, 3)), np.zeros(ns), np.zeros((ns, 16))
        bi, it = np.zeros(ns, np.int32), np.zeros(ns, np.int32)
        check(lib().mcs_sim3_best(self.h, np_ptr(R), np_ptr(t), np_ptr(s), np_ptr(T), np_ptr(bi), np_ptr(it)))
        return R.reshape(ns, 3, 3), t, s, T.reshape(ns, 4, 4), bi, it

    def info(self):
        """-> (N, mRansacMaxIts, mnIterations) per solver"""
        ns = len(self.solvers)
        n, mx, it = np.zeros(ns, np.int32), np.zeros(ns, np.int32), np.zeros(ns, np.int32)
        check(lib().mcs_sim3_info(self.h, np_ptr(n), np_ptr(mx), np_ptr(it)))
        return n, mx, it

    def hypotheses(self, solver, first, count, masks=True):
        """diagnostics: the hypotheses of iterations [first, first + count) of one solver -> dict(picks [count,3], n_inliers [count],
        T12 / T21 [count,4,4], R [count,3,3], t [count,3], s [count], inliers [count,N] bool or None)"""
        N = int(self.solvers[solver].N)
        picks, cnt, hyp = np.zeros((max(count, 1), 3), np.int32), np.zeros(max(count, 1), np.int32), np.zeros((max(count, 1), 45))
        inl = np.zeros((max(count, 1), max(N, 1)), np.uint8) if masks else None
        check(lib().mcs_sim3_hypotheses(self.h, int(solver), int(first), int(count), np_ptr(picks), np_ptr(cnt), np_ptr(hyp), np_ptr(inl)))
        hyp = hyp[:count]
        return dict(picks=picks[:count], n_inliers=cnt[:count], T12=hyp[:, :16].reshape(-1, 4, 4), T21=hyp[:, 16:32].reshape(-1, 4, 4),
                    R=hyp[:, 32:41].reshape(-1, 3, 3), t=hyp[:, 41:44], s=hyp[:, 44], inliers=None if inl is None else inl[:count, :N].astype(bool))


class cSim3Solver:
    """cSim3Solver (include/cSim3Solver.h, src/cSim3Solver.cpp): the constructor's pointer filtering runs here, everything numeric in the library
    (mcs_sim3_*).  Keyframes need GetMapPointMatches(), GetKeyPoint(i)["octave"], GetSigma2(level), keypoint_to_cam and camSystem (M_t_inv,
    MtMc_inv); map points isBad(), GetIndexInKeyFrame(pKF), GetWorldPos().  camSys: the local rig (cMultiCamSys_, its M_c and camera models)."""

    def __init__(self, pKF1, pKF2, vpMatched12, camSys, ctx=None, seed=0):
        self.ctx = ctx or default_context()
        self.seed = int(seed)
        self.camSysLocal = camSys
        self.mpKF1, self.mpKF2 = pKF1, pKF2
        self.mvpMatches12 = list(vpMatched12)
        self.mN1 = len(self.mvpMatches12)
        vpKeyFrameMP1 = pKF1.GetMapPointMatches()
        X, cams, sig, idx1 = [], [], [], []
        for i1, pMP2 in enumerate(self.mvpMatches12):   # :71-134
            if pMP2 is None:
                continue
            pMP1 = vpKeyFrameMP1[i1]
            if pMP1 is None:
                continue
            if pMP1.isBad() or pMP2.isBad():
                continue
            idxs1, idxs2 = pMP1.GetIndexInKeyFrame(pKF1), pMP2.GetIndexInKeyFrame(pKF2)
            if len(idxs1) == 0 or len(idxs2) == 0:
                continue
            indexKF1, indexKF2 = int(idxs1[0]), int(idxs2[0])   # the first index only
            if indexKF1 < 0 or indexKF2 < 0:
                continue
            sig.append((float(pKF1.GetSigma2(int(pKF1.GetKeyPoint(indexKF1)["octave"]))), float(pKF2.GetSigma2(int(pKF2.GetKeyPoint(indexKF2)["octave"])))))
            cams.append((int(pKF1.keypoint_to_cam[indexKF1]), int(pKF2.keypoint_to_cam[indexKF2])))
            X.append(np.concatenate([np.asarray(pMP1.GetWorldPos(), np.float64).reshape(-1)[:3], np.asarray(pMP2.GetWorldPos(), np.float64).reshape(-1)[:3]]))
            idx1.append(i1)
        self.N = len(idx1)
        self._Xw = np.asarray(X, np.float64).reshape(self.N, 2, 3)
        self._cam = np.asarray(cams, np.int32).reshape(self.N, 2)
        self._sig = np.asarray(sig, np.float64).reshape(self.N, 2)
        self._idx1 = np.asarray(idx1, np.int32)
        self.mvnIndices1 = self._idx1
        nr = camSys.GetNrCams()
        self._Mt = np.stack([np.asarray(k.camSystem.M_t_inv, np.float64).reshape(16) for k in (pKF1, pKF2)])
        self._MtMc = np.stack([np.stack([np.asarray(m, np.float64).reshape(16) for m in k.camSystem.MtMc_inv[:nr]]) for k in (pKF1, pKF2)])
        self._batch, self._slot = None, 0
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):   # :139-165
        self.mRansacProb, self.mRansacMinInliers, self.mRansacMaxItsParam = float(probability), int(minInliers), int(maxIterations)
        if self._batch is not None:
            self._batch.SetRansacParameters()

    def _b(self):
        if self._batch is None:
            cSim3SolverBatch([self], self.ctx, self.seed)
        return self._batch

    def iterate(self, nIterations):
        """-> (success, bNoMore, vbInliers [mN1] bool, nInliers, T12 4x4 or None)"""
        b = self._b()
        n = [0] * len(b.solvers)
        n[self._slot] = int(nIterations)
        return b.iterate(n)[self._slot]

    def find(self):   # :256-262 -> (success, vbInliers12, nInliers, T12)
        b = self._b()
        mx = int(b.info()[1][self._slot])
        ok, _, vb, n, T = self.iterate(mx)
        return ok, vb, n, T

    def GetEstimatedRotation(self):
        return self._b().best()[0][self._slot]

    def GetEstimatedTranslation(self):
        return self._b().best()[1][self._slot]

    def GetEstimatedScale(self):
        return float(self._b().best()[2][self._slot])


# ---------------------------------------------------------------------------------------------- the local map and the covisibility counts (mcs_covis_*)
_hiprt = None


def _hip():
    """the HIP runtime libmcs_hip.so is linked with (already in the process): device arrays for the device-kind chain of TrackLocalMapSearch"""
    global _hiprt
    if _hiprt is None:
        lib()
        _hiprt = C.CDLL("libamdhip64.so")
        _hiprt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hiprt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hiprt.hipFree.argtypes = [C.c_void_p]
    return _hiprt


class DeviceArray:
    """a numpy array's copy in device memory: .ptr for device-kind calls, .read() synchronises and copies it back"""

    def __init__(self, arr):
        self.arr = np.ascontiguousarray(arr)
        self.ptr = C.c_void_p()
        if _hip().hipMalloc(C.byref(self.ptr), max(self.arr.nbytes, 16)) != 0:
            raise MemoryError("hipMalloc of %d bytes failed" % self.arr.nbytes)
        if self.arr.nbytes and _hip().hipMemcpy(self.ptr, self.arr.ctypes.data_as(C.c_void_p), self.arr.nbytes, 1) != 0:
            raise RuntimeError("hipMemcpy to the device failed")

    def read(self):
        out = np.empty_like(self.arr)
        if _hip().hipDeviceSynchronize() != 0 or (out.nbytes and _hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes, 2) != 0):
            raise RuntimeError("hipMemcpy from the device failed")
        return out

    def __del__(self):
        try:
            if self.ptr:
                _hip().hipFree(self.ptr)
        except Exception:
            pass


def _point_ids(points):
    """mvpMapPoints as ids: None / -1 -> -1, an int, or a map point's mnId"""
    return np.array([-1 if m is None else int(getattr(m, "mnId", m)) for m in points], np.int32)


def _kf_id(kf):
    return int(getattr(kf, "mnId", kf))


class cCovisibility:
    """The observation store behind cTracking::UpdateReferenceKeyFrames / UpdateReferencePoints (src/cTracking.cpp:1024-1123) and
    cMultiKeyFrame::UpdateConnections (src/cMultiKeyFrame.cpp:406-500) on the device (mcs_covis_*), and behind cLocalMapping::KeyFrameCulling / MapPointCulling
    (src/cLocalMapping.cpp:517-593, 187-221): one row of map point ids (and one of octaves) per keyframe.  Keyframes are
    objects with mnId (and GetMapPointMatches() / GetCameraCenter() where no array is given) or plain ids; map points are objects with mnId or plain ids
    in [0, max_points).  Where the reference orders by heap address the store orders by mnId."""

    def __init__(self, max_keyframes, max_features, max_points, ctx=None):
        self.ctx = ctx or default_context()
        self.h = C.c_void_p()
        check(lib().mcs_covis_create(self.ctx.h, int(max_keyframes), int(max_features), int(max_points), C.byref(self.h)))
        self.max_points = int(max_points)
        self.slot_ids = []   # mnId of every slot, erased ones included (slot order is id order)

    def __del__(self):
        try:
            if self.h:
                lib().mcs_covis_destroy(self.h)
        except Exception:
            pass

    def _n(self, fn):
        n = C.c_int32()
        check(fn(self.h, C.byref(n)))
        return n.value

    def size(self):
        return self._n(lib().mcs_covis_size)

    def slots(self):
        return self._n(lib().mcs_covis_slots)

    def clear(self):
        check(lib().mcs_covis_clear(self.h))
        self.slot_ids = []

    def SetKeyFrame(self, pKF, points=None):
        """add the keyframe or replace its row (points: default pKF.GetMapPointMatches())"""
        ids = _point_ids(pKF.GetMapPointMatches() if points is None else points)
        check(lib().mcs_covis_set_keyframe(self.h, _kf_id(pKF), np_ptr(ids), len(ids), MEM_HOST))
        if not self.slot_ids or _kf_id(pKF) > self.slot_ids[-1]:
            self.slot_ids.append(_kf_id(pKF))

    def SetPose(self, kfs, ts=None):
        """Hom2T(GetPose()) of the listed keyframes (ts: default their GetCameraCenter())"""
        kfs = list(kfs)
        ids = np.array([_kf_id(k) for k in kfs], np.int64)
        t = np.ascontiguousarray([np.asarray(k.GetCameraCenter(), np.float64).reshape(-1)[:3] for k in kfs] if ts is None else ts, np.float64).reshape(len(kfs), 3)
        check(lib().mcs_covis_set_keyframe_pose(self.h, len(kfs), np_ptr(ids), np_ptr(t), MEM_HOST))

    def EraseKeyFrame(self, pKF):
        check(lib().mcs_covis_erase_keyframe(self.h, _kf_id(pKF)))

    def SetBadFlag(self, pKF, bad=True):
        check(lib().mcs_covis_set_keyframe_bad(self.h, _kf_id(pKF), int(bool(bad))))

    def SetPointsBad(self, points, bad=True):
        ids = _point_ids(points)
        flags = np.ascontiguousarray(np.broadcast_to(np.asarray(bad, bool), ids.shape), np.uint8)
        check(lib().mcs_covis_set_points_bad(self.h, np_ptr(ids), len(ids), np_ptr(flags), MEM_HOST))

    def UpdateReference(self, F, frame_t=None, cap=None):
        """UpdateReferenceKeyFrames + UpdateReferencePoints for frame F: an object with mvpMapPoints (entries of bad points become None, as in the reference) and
        camSystem.M_t, or an array of point ids together with frame_t.  -> dict(frame_points, local_kfs, weights, dists, ref_kf (-1: none), local_points,
        n_points); n_points above cap means the list was cut at cap."""
        obj = hasattr(F, "mvpMapPoints")
        fp = _point_ids(F.mvpMapPoints if obj else F)
        t = np.ascontiguousarray(np.asarray(F.camSystem.M_t, np.float64)[:3, 3] if frame_t is None else frame_t, np.float64).reshape(3)
        S = self.slots()
        cap = self.max_points if cap is None else int(cap)
        kfs, w, d = np.zeros(max(S, 1), np.int64), np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1))
        nl, ref, npnt = np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.int32)
        lp = np.zeros(max(cap, 1), np.int32)
        check(lib().mcs_covis_update_reference(self.h, np_ptr(fp), len(fp), np_ptr(t), cap, MEM_HOST, np_ptr(kfs), np_ptr(w), np_ptr(d), np_ptr(nl), np_ptr(ref),
                                               np_ptr(lp), np_ptr(npnt)))
        if obj:
            for i in np.flatnonzero(fp < 0):
                F.mvpMapPoints[int(i)] = None
        n = int(nl[0])
        return dict(frame_points=fp, local_kfs=kfs[:n].tolist(), weights=w[:n].tolist(), dists=d[:n].tolist(), ref_kf=int(ref[0]),
                    local_points=lp[:min(int(npnt[0]), cap)].tolist(), n_points=int(npnt[0]))

    def UpdateConnections(self, kfs):
        """the counting and ordering of UpdateConnections for every listed keyframe, in one call -> per keyframe dict(counter {mnId: count}, ordered, weights);
        ordered / weights are None where KFcounter is empty (the reference leaves its lists unchanged).  ordered[:N] is GetBestCovisibilityKeyFrames(N)."""
        kfs = list(kfs)
        nq, S = len(kfs), self.slots()
        if nq == 0:
            return []
        ids = np.array([_kf_id(k) for k in kfs], np.int64)
        cnt, nc = np.zeros(nq * S, np.int32), np.zeros(nq, np.int32)
        od, ow, no = np.zeros(nq * S, np.int64), np.zeros(nq * S, np.int32), np.zeros(nq, np.int32)
        check(lib().mcs_covis_update_connections(self.h, nq, np_ptr(ids), MEM_HOST, np_ptr(cnt), np_ptr(nc), np_ptr(od), np_ptr(ow), np_ptr(no)))
        out = []
        for q in range(nq):
            n, c = int(no[q]), cnt[q * S:(q + 1) * S]
            counter = {self.slot_ids[int(k)]: int(c[k]) for k in np.flatnonzero(c)}   # KFcounter: the counts come per slot
            assert len(counter) == int(nc[q])
            out.append(dict(counter=counter, ordered=None if n < 0 else od[q * S:q * S + n].tolist(), weights=None if n < 0 else ow[q * S:q * S + n].tolist()))
        return out

    # ---- cLocalMapping::KeyFrameCulling / MapPointCulling (src/cLocalMapping.cpp:517-593, 187-221).  device=True: the same call device-kind — inputs and outputs
    # in device memory, nothing read back before the call has returned (the pattern of TrackLocalMapSearch) — with the same results.
    def _arrays(self, device, ins, outs):
        """-> (pointers of ins + outs, reader of the outs)"""
        mem = _DEVICE if device else _HOST
        d = [mem.put(a) for a in list(ins) + list(outs)]
        return [mem.ptr(x) for x in d], lambda: [mem.read(x) for x in d[len(ins):]]

    def SetOctaves(self, pKF, octaves=None, device=False):
        """octaves[i] = pKF.GetKeyPoint(i).octave (default: the keyframe's keypoints)"""
        o = np.ascontiguousarray(pKF.GetKeyPoints()["octave"] if octaves is None else octaves).astype(np.uint8)
        (po,), _ = self._arrays(device, [o], [])
        check(lib().mcs_covis_set_keyframe_octaves(self.h, _kf_id(pKF), po, len(o), MEM_DEVICE if device else MEM_HOST))

    def KeyFrameCulling(self, kfs, not_erase=None, cap=None, device=False):
        """kfs: mpCurrentMultiKeyFrame->GetVectorCovisibleKeyFrames(), in that order; not_erase: mbNotErase per keyframe (default: the keyframes' attribute, False
        where there is none).  -> dict(verdict (0 kept, 1 culled, 2 to be erased, 3 mnId == 0), n_mps, n_redundant, culled / to_be_erased (the entries of kfs),
        bad_points, n_bad_points (above cap: the list was cut)).  Culled keyframes and bad points are flagged in the store; the keyframes are NOT erased:
        EraseKeyFrame them, and do the spanning-tree / map / database part of cMultiKeyFrame::SetBadFlag, once the verdicts are here."""
        kfs = list(kfs)
        n = len(kfs)
        cap = self.max_points if cap is None else int(cap)
        ids = np.array([_kf_id(k) for k in kfs], np.int64)
        ne = np.array([bool(getattr(k, "mbNotErase", False)) for k in kfs] if not_erase is None else not_erase, np.uint8).reshape(n)
        outs = [np.zeros(max(n, 1), np.int32) for _ in range(3)] + [np.zeros(max(cap, 1), np.int32), np.zeros(1, np.int32)]
        ptr, read = self._arrays(device, [], outs)
        check(lib().mcs_covis_cull_keyframes(self.h, n, np_ptr(ids), np_ptr(ne), cap, MEM_DEVICE if device else MEM_HOST, *ptr))
        v, m, r, bp, nb = read()
        v = v[:n].tolist()
        return dict(verdict=v, n_mps=m[:n].tolist(), n_redundant=r[:n].tolist(), culled=[k for k, x in zip(kfs, v) if x == 1],
                    to_be_erased=[k for k, x in zip(kfs, v) if x == 2], bad_points=bp[:min(int(nb[0]), cap)].tolist(), n_bad_points=int(nb[0]))

    def Observations(self, points, device=False):
        """cMapPoint::Observations() of the listed points: the live keyframes whose row holds the point, 0 for a bad one"""
        ids = _point_ids(points)
        if len(ids) == 0:
            return []
        ptr, read = self._arrays(device, [ids], [np.zeros(len(ids), np.int32)])
        check(lib().mcs_covis_observations(self.h, ptr[0], len(ids), MEM_DEVICE if device else MEM_HOST, ptr[1]))
        return read()[0].tolist()

    def MapPointCulling(self, current_kf, points, found, visible, first_kf, device=False):
        """points: mlpRecentAddedMapPoints (distinct) with mnFound / mnVisible / mnFirstKFid per entry -> (verdicts, the list that remains).  Verdicts: 0 stays,
        1 was bad, 2 found ratio below a quarter (now bad), 3 two or fewer observations after two keyframes (now bad), 4 three keyframes old."""
        points = list(points)
        ids = _point_ids(points)
        n = len(ids)
        if n == 0:
            return [], []
        ins = [ids, np.ascontiguousarray(found, np.int32).reshape(n), np.ascontiguousarray(visible, np.int32).reshape(n),
               np.array([int(k) for k in first_kf], np.int64).reshape(n)]
        ptr, read = self._arrays(device, ins, [np.zeros(n, np.int32)])
        check(lib().mcs_covis_cull_points(self.h, _kf_id(current_kf), n, ptr[0], ptr[1], ptr[2], ptr[3], MEM_DEVICE if device else MEM_HOST, ptr[4]))
        v = read()[0].tolist()
        return v, [p for p, x in zip(points, v) if x == 0]


    # ---- cMapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors (src/cMapPoint.cpp:449-492, 294-388) over the store
    def SetDescriptors(self, pKF, desc=None, mask=None, device=False):
        """the keyframe's descriptor (and mask) rows in continuous feature-index order.  desc=None: the keyframe's own rows (a cMultiKeyFrame's flat copies, or
        all_descriptors() / all_masks()), with its masks unless mask=False; the first call fixes the row width and whether masks exist for the whole store"""
        if desc is None:
            desc = pKF._d if hasattr(pKF, "_d") else pKF.all_descriptors()
            if mask is None:
                mask = pKF._m if hasattr(pKF, "_m") else pKF.all_masks()
        if mask is False:
            mask = None
        d = np.ascontiguousarray(desc, np.uint8)
        d = d.reshape(len(d), -1)
        ins = [d] + ([np.ascontiguousarray(mask, np.uint8).reshape(d.shape)] if mask is not None else [])
        ptr, _ = self._arrays(device, ins, [])
        check(lib().mcs_covis_set_keyframe_descriptors(self.h, _kf_id(pKF), ptr[0], ptr[1] if mask is not None else None, d.shape[1], d.shape[1], len(d),
                                                        MEM_DEVICE if device else MEM_HOST))

    UPDATE_OUTPUTS = ("normal", "min_dist", "max_dist", "min_inv", "max_inv", "desc", "mask", "n_desc", "best_kf", "best_feat", "status")

    def UpdateMapPoints(self, points, pos, ref_kf, scale_factors, desc=None, mask=None, device=False, init=None, skip=()):
        """UpdateNormalAndDepth + ComputeDistinctiveDescriptors for the listed points.  pos [n][3]; ref_kf: mpRefKF per point (keyframes or ids); desc (/ mask)
        [n][dim]: the points' current descriptors, kept where none is chosen — desc=None refreshes normal and depth only.  init: {output: array} to start an
        output from (entries whose status is not 0 keep it; default zeros, -1 for best_kf / best_feat); skip: outputs passed as NULL.
        -> dict of the outputs (list-indexed): normal, min_dist, max_dist, min_inv, max_inv, [desc, mask, n_desc, best_kf, best_feat,] status"""
        ids = _point_ids(points)
        n = len(ids)
        sf = np.ascontiguousarray(scale_factors, np.float64).reshape(-1)
        m = max(n, 1)
        ins = [ids, np.ascontiguousarray(pos, np.float64).reshape(n, 3), np.array([_kf_id(k) for k in ref_kf], np.int64).reshape(n), sf]
        outs = dict(normal=np.zeros((m, 3)), min_dist=np.zeros(m), max_dist=np.zeros(m), min_inv=np.zeros(m), max_inv=np.zeros(m), status=np.zeros(m, np.int32))
        if desc is not None:
            d = np.ascontiguousarray(desc, np.uint8)
            d = d.reshape(n, d.size // m)
            outs.update(desc=d.copy(), n_desc=np.zeros(m, np.int32), best_kf=np.full(m, -1, np.int64), best_feat=np.full(m, -1, np.int32))
            if mask is not None:
                outs["mask"] = np.ascontiguousarray(mask, np.uint8).reshape(d.shape).copy()
        for k, a in (init or {}).items():
            if k in outs:
                outs[k] = np.ascontiguousarray(a, outs[k].dtype).reshape(outs[k].shape).copy()
        names = [k for k in self.UPDATE_OUTPUTS if k in outs and k not in skip]
        ptr, read = self._arrays(device, ins, [outs[k] for k in names])
        at = dict(zip(names, ptr[4:]))
        check(lib().mcs_covis_update_points(self.h, n, ptr[0], ptr[1], ptr[2], ptr[3], len(sf), MEM_DEVICE if device else MEM_HOST,
                                            *[at.get(k) for k in self.UPDATE_OUTPUTS]))
        return {k: a[:n] for k, a in zip(names, read())}


def TrackLocalMapSearch(F, store, points, th=3, nnratio=0.8, featDim=32, havingMasks=False, cap=None, ctx=None):
    """The first two steps of cTracking::TrackLocalMap (src/cTracking.cpp:834-848) as ONE chain of device-kind calls, nothing in between visiting the host:
    mcs_covis_update_reference -> mcs_gather_rows of the per-point tables through the local list -> mcs_search_local_points on the padded list (n = cap) ->
    mcs_scatter_rows of the tracking state.
    F: a cMultiFrame whose mvpMapPoints holds map point ids (or objects with mnId) or None.  points: the per-point tables indexed by map point id —
    pos / normal [n][3], min_dist / max_dist [n], flags [n] (LP_BAD; LP_SEEN is set here), desc (/ mask) [n][featDim], in_view / proj_x / proj_y / level /
    view_cos [n][nr_cams]; the tracking state is updated in place.  The frame's first loop (:957-976) runs here on the arrays.
    -> dict(nmatches (the reference's return value), n_to_match, local_kfs, weights, dists, ref_kf, local_points, n_points, match [cap][nr_cams],
    visible_inc [n] (IncreaseVisible() calls per point id, first loop included), frame_points)"""
    from ._capi import LP_BAD, LP_SEEN, LocalPoints, TrackState
    ctx = ctx or store.ctx
    L = lib()
    nr = F.camSystem.GetNrCams()
    npts = len(points["flags"])
    cap = npts if cap is None else int(cap)
    fp = _point_ids(F.mvpMapPoints)
    fcam = np.ascontiguousarray(F.keypoint_to_cam, np.int32)
    flags = np.ascontiguousarray(points["flags"], np.uint8).copy()
    vis_first = np.zeros(npts, np.int32)
    first = 0
    for i in np.flatnonzero(fp >= 0):                 # :957-976 (the entries of bad points are nulled by the device call below, as :1072-1075 did before)
        p = int(fp[i])
        if flags[p] & LP_BAD:
            continue
        vis_first[p] += 1
        flags[p] |= LP_SEEN
        points["in_view"][p, int(fcam[i])] = 0
        first += 1
    assigned = np.array([p >= 0 and not (flags[p] & LP_BAD) for p in fp] or [0], np.uint8)
    S = store.slots()
    dev = DeviceArray
    tab = {k: dev(np.ascontiguousarray(points[k], dt)) for k, dt in (("pos", np.float64), ("normal", np.float64), ("min_dist", np.float64), ("max_dist", np.float64),
                                                                  ("desc", np.uint8), ("in_view", np.uint8), ("proj_x", np.float64), ("proj_y", np.float64),
                                                                  ("level", np.int32), ("view_cos", np.float64))}
    tab["flags"] = dev(flags)
    if havingMasks:
        tab["mask"] = dev(np.ascontiguousarray(points["mask"], np.uint8))
    d_fp, d_t = dev(fp), dev(np.ascontiguousarray(np.asarray(F.camSystem.M_t, np.float64)[:3, 3]))
    o = dict(kfs=dev(np.zeros(max(S, 1), np.int64)), w=dev(np.zeros(max(S, 1), np.int32)), d=dev(np.zeros(max(S, 1))), nl=dev(np.zeros(1, np.int32)),
             ref=dev(np.zeros(1, np.int64)), lp=dev(np.zeros(max(cap, 1), np.int32)), np=dev(np.zeros(1, np.int32)))
    check(L.mcs_covis_update_reference(store.h, d_fp.ptr, len(fp), d_t.ptr, cap, MEM_DEVICE, o["kfs"].ptr, o["w"].ptr, o["d"].ptr, o["nl"].ptr, o["ref"].ptr,
                                       o["lp"].ptr, o["np"].ptr))
    g = {}
    for k, a in tab.items():                          # the padded local list: row i = the table's row local_points[i]; the padding reads "bad"
        row = a.arr.nbytes // max(npts, 1)
        g[k] = dev(np.zeros((max(cap, 1),) + a.arr.shape[1:], a.arr.dtype))
        fill = np.array([LP_BAD], np.uint8) if k == "flags" else None
        check(L.mcs_gather_rows(ctx.h, o["lp"].ptr, cap, a.ptr, row, np_ptr(fill), g[k].ptr))
    rv, keep = _rig_view(F.camSystem, _DEVICE)
    lpv = LocalPoints(g["pos"].ptr, g["normal"].ptr, g["min_dist"].ptr, g["max_dist"].ptr, g["flags"].ptr, cap)
    ts = TrackState(*[g[k].ptr for k in ("in_view", "proj_x", "proj_y", "level", "view_cos")])
    fv, fa = _frame_view(F, featDim, havingMasks, assigned, _DEVICE)
    res = dict(match=dev(np.full(max(cap * nr, 1), -1, np.int32)), nm=dev(np.zeros(1, np.int32)), ntm=dev(np.zeros(1, np.int32)), vis=dev(np.zeros(max(cap, 1), np.int32)))
    check(L.mcs_search_local_points(ctx.h, C.byref(lpv), C.byref(rv), C.byref(ts), g["desc"].ptr, g["mask"].ptr if havingMasks else None, featDim, C.byref(fv),
                                    float(th), float(nnratio), featDim, MEM_DEVICE, res["match"].ptr, res["nm"].ptr, res["ntm"].ptr, res["vis"].ptr))
    for k in ("in_view", "proj_x", "proj_y", "level", "view_cos"):
        check(L.mcs_scatter_rows(ctx.h, o["lp"].ptr, cap, g[k].ptr, tab[k].arr.nbytes // max(npts, 1), tab[k].ptr))
    # ---- only now the host looks at anything
    n_points = int(o["np"].read()[0])
    lp = o["lp"].read()[:cap]
    for k in ("in_view", "proj_x", "proj_y", "level", "view_cos"):
        points[k][...] = tab[k].read().reshape(points[k].shape)
    vis = vis_first.copy()
    used = min(n_points, cap)
    np.add.at(vis, lp[:used], res["vis"].read()[:used])
    n = int(o["nl"].read()[0])
    fp_after = d_fp.read()
    match = res["match"].read()[:cap * nr].reshape(cap, nr)
    for i in np.flatnonzero(fp_after < 0):
        F.mvpMapPoints[int(i)] = None
    for i, c in zip(*np.nonzero(match >= 0)):
        F.mvpMapPoints[int(match[i, c])] = int(lp[i])            # F.mvpMapPoints[bestIdx] = pMP, src/cORBmatcher.cpp:159
    nm = int(res["nm"].read()[0])
    return dict(nmatches=first + nm, search_matches=nm, n_to_match=int(res["ntm"].read()[0]), local_kfs=o["kfs"].read()[:n].tolist(), weights=o["w"].read()[:n].tolist(),
                dists=o["d"].read()[:n].tolist(), ref_kf=int(o["ref"].read()[0]), local_points=lp[:used].tolist(), n_points=n_points, match=match,
                visible_inc=vis, search_visible_inc=res["vis"].read()[:cap], frame_points=fp_after)


# ---------------------------------------------------------------------------------------------- the frame-to-frame searches of the tracker, one device call each
def _tracked_call(Fs, Ft, points, featDim, havingMasks, device, rig_of=None):
    """the arrays of mcs_tracked_frame (Ft: the frame whose points are carried over), mcs_point_table, mcs_frame_view (Fs: the frame searched in) and, with
    rig_of, mcs_rig_view, in host or device memory -> (structs, arrays by name, keepalive, the memory)"""
    from ._capi import PointTable, TrackedFrame
    mem = _DEVICE if device else _HOST
    a = dict(tkeys=Ft.mvKeys, tdesc=np.asarray(Ft.all_descriptors(), np.uint8), tmask=np.asarray(Ft.all_masks(), np.uint8) if havingMasks else None,
             tcam=np.asarray(Ft.keypoint_to_cam, np.int32), tpoints=_point_ids(Ft.mvpMapPoints),
             toutlier=np.asarray(getattr(Ft, "mvbOutlier", np.zeros(Ft.totalN)), np.uint8), pos=np.asarray(points["pos"], np.float64),
             flags=np.asarray(points["flags"], np.uint8))
    a = {k: mem.put(v) for k, v in a.items()}
    tf = TrackedFrame(*[mem.ptr(a[k]) for k in ("tkeys", "tdesc", "tmask", "tcam", "tpoints", "toutlier")], Ft.totalN, featDim)
    tab = PointTable(mem.ptr(a["pos"]), mem.ptr(a["flags"]), len(points["flags"]))
    fv, fa = _frame_view(Fs, featDim, havingMasks, np.array([m is not None for m in Fs.mvpMapPoints] or [0], np.uint8), mem)
    a.update(fa)
    rv, keep = _rig_view(rig_of, mem) if rig_of is not None else (None, [])
    return (tf, tab, fv, rv), a, keep, mem


def _track_outputs(n, mem, entry_points=None):
    return dict(match=mem.put(np.full(max(n, 1), -1, np.int32)), points=mem.put(np.full(max(n, 1), -1, np.int32) if entry_points is None else entry_points),
                nm=mem.put(np.zeros(1, np.int32)))


def TrackWithMotionModelSearch(Cur, Last, points, th, featDim=32, havingMasks=False, checkOrientation=False, device=False, ctx=None):
    """The search of cTracking::TrackWithMotionModel, cORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) (src/cORBmatcher.cpp:1990-2118), as ONE
    call (mcs_search_last_frame); device=True: device kind — every array in device memory, nothing read back before the call has returned (the pattern of
    TrackLocalMapSearch).  Cur / Last: cMultiFrames whose mvpMapPoints hold map point ids (or objects with mnId) or None; Last.mvbOutlier per feature.
    points: the per-id tables pos [n][3] and flags [n] (LP_BAD).  Cur.mvpMapPoints receives the ids of the new matches.
    -> dict(nmatches, match_cur, cur_points, assigned)"""
    ctx = ctx or default_context()
    (tf, tab, fv, rv), a, keep, mem = _tracked_call(Cur, Last, points, featDim, havingMasks, device, Cur.camSystem)
    n = Cur.totalN
    o = _track_outputs(n, mem, np.resize(_point_ids(Cur.mvpMapPoints), max(n, 1)).astype(np.int32))
    check(lib().mcs_search_last_frame(ctx.h, C.byref(tf), C.byref(tab), C.byref(rv), C.byref(fv), float(th), featDim, int(bool(checkOrientation)), mem.kind,
                                      mem.ptr(o["match"]), mem.ptr(o["points"]), mem.ptr(o["nm"])))
    # ---- only now the host looks at anything
    match, cp, asg = mem.read(o["match"])[:n], mem.read(o["points"])[:n], mem.read(a["assigned"])[:n]
    for j in np.flatnonzero(match >= 0):
        Cur.mvpMapPoints[int(j)] = int(cp[j])          # CurrentFrame.mvpMapPoints[bestIdx2] = pMP, :2075
    return dict(nmatches=int(mem.read(o["nm"])[0]), match_cur=match, cur_points=cp, assigned=asg)


def TrackPreviousFrameWindowSearch(Last, Cur, points, windowSize, minScaleLevel=0, maxScaleLevel=2**31 - 1, nnratio=0.8, featDim=32, havingMasks=False,
                                   checkOrientation=False, device=False, ctx=None):
    """The first search of cTracking::TrackPreviousFrame, cORBmatcher::WindowSearch(LastFrame, CurrentFrame, windowSize, vpMapPointMatches, minScaleLevel,
    maxScaleLevel) (src/cORBmatcher.cpp:326-473), as ONE call (mcs_window_search_frames); frames and tables as for TrackWithMotionModelSearch (Cur's own
    matches and Last.mvbOutlier are not read, as in the reference).  Cur.mvpMapPoints becomes vpMapPointMatches2 (ids, None where unmatched), which is what
    TrackPreviousFrame assigns (src/cTracking.cpp:751).  -> dict(nmatches, match21, points2)"""
    ctx = ctx or default_context()
    (tf, tab, fv, rv), a, keep, mem = _tracked_call(Cur, Last, points, featDim, havingMasks, device)
    n = Cur.totalN
    o = _track_outputs(n, mem)
    check(lib().mcs_window_search_frames(ctx.h, C.byref(tf), C.byref(tab), C.byref(fv), int(windowSize), int(minScaleLevel), int(min(maxScaleLevel, 2**31 - 1)),
                                         float(nnratio), featDim, int(bool(checkOrientation)), mem.kind, mem.ptr(o["match"]), mem.ptr(o["points"]),
                                         mem.ptr(o["nm"])))
    match, p2 = mem.read(o["match"])[:n], mem.read(o["points"])[:n]
    Cur.mvpMapPoints = [int(p) if p >= 0 else None for p in p2]
    return dict(nmatches=int(mem.read(o["nm"])[0]), match21=match, points2=p2)


# ---------------------------------------------------------------------------------------------- the frame's pose (mcs_pose_optimization)
def PoseOptimizationBatch(frames, points, huberMultiplier=1.0, device=False, ctx=None, diag=False):
    """cOptimizer::PoseOptimization (src/cOptimizer.cpp:259-459) for a list of frames that share one rig model (cameras, M_c) and one point table, as ONE call
    (mcs_pose_optimization).  Every frame: mvKeys, keypoint_to_cam, mvpMapPoints (ids, objects with mnId, or None), mvInvLevelSigma2, camSystem (GetPoseMin,
    Get_M_c_min).  points: dict(pos [n][3]).  huberMultiplier: one value or one per frame.  device=True: every array in device memory, nothing read back before
    the call has returned.  Sets F.mvbOutlier and the frame's rig through Set_M_t_from_min, with MtMc / MtMc_inv as the device built them.
    -> [(nInliers, outlierShare)] per frame; diag=True: (that list, the mcs_pose_diag records)"""
    from ._capi import POSE_DIAG_DTYPE, PointTable, PoseFrame
    ctx = ctx or default_context()
    npb = len(frames)
    if npb == 0:
        check(lib().mcs_pose_optimization(ctx.h, 0, None, None, None, None, 0, None, 0, None, MEM_HOST, None, None, None, None, None, None, None))
        return ([], np.zeros(0, POSE_DIAG_DTYPE)) if diag else []
    mem = _DEVICE if device else _HOST
    rig = frames[0].camSystem
    nr = rig.GetNrCams()
    ocs = (type(rig.cams[0].ocam) * nr)(*[cm.ocam for cm in rig.cams])
    sig = np.asarray(frames[0].mvInvLevelSigma2, np.float64)
    hub = np.resize(np.asarray(huberMultiplier, np.float64), npb).astype(np.float64)
    pos = np.ascontiguousarray(points["pos"], np.float64).reshape(-1, 3)
    g = dict(pos=pos, Mc=np.ascontiguousarray([rig.Get_M_c_min(c) for c in range(nr)], np.float64), ocs=np.frombuffer(ocs, np.uint8).copy(), sig=sig, hub=hub,
             pose=np.ascontiguousarray([F.camSystem.GetPoseMin() for F in frames], np.float64), MtMc=np.zeros((npb, nr, 16)), inv=np.zeros((npb, nr, 16)),
             nin=np.zeros(npb, np.int32), share=np.zeros(npb), diag=np.zeros(npb, POSE_DIAG_DTYPE))
    g = {k: mem.put(v) for k, v in g.items()}
    per = [dict(keys=mem.put(F.mvKeys), cam=mem.put(np.asarray(F.keypoint_to_cam, np.int32)), points=mem.put(_point_ids(F.mvpMapPoints)),
                out=mem.put(np.zeros(max(len(F.mvpMapPoints), 1), np.uint8))) for F in frames]
    fr = (PoseFrame * npb)(*[PoseFrame(mem.ptr(q["keys"]), mem.ptr(q["cam"]), mem.ptr(q["points"]), len(F.mvpMapPoints)) for q, F in zip(per, frames)])
    outs = (C.c_void_p * npb)(*[mem.ptr(q["out"]) for q in per])
    tab = PointTable(mem.ptr(g["pos"]), None, len(pos))
    check(lib().mcs_pose_optimization(ctx.h, npb, fr, C.byref(tab), mem.ptr(g["Mc"]), mem.ptr(g["ocs"]), nr, mem.ptr(g["sig"]), len(sig), mem.ptr(g["hub"]), mem.kind,
                                      mem.ptr(g["pose"]), mem.ptr(g["MtMc"]), mem.ptr(g["inv"]), outs, mem.ptr(g["nin"]), mem.ptr(g["share"]), mem.ptr(g["diag"])))
    # ---- only now the host looks at anything
    pose, MtMc, inv, nin, share = (mem.read(g[k]) for k in ("pose", "MtMc", "inv", "nin", "share"))
    res = []
    for p, (F, q) in enumerate(zip(frames, per)):
        n = len(F.mvpMapPoints)
        F.mvbOutlier = [bool(v) for v in mem.read(q["out"])[:n]]
        F.camSystem.Set_M_t_from_min(pose[p], MtMc[p], inv[p])
        res.append((int(nin[p]), float(share[p])))
    return (res, mem.read(g["diag"])) if diag else res


def PoseOptimization(F, points, huberMultiplier=1.0, device=False, ctx=None):
    """int cOptimizer::PoseOptimization(cMultiFrame* pFrame, double& inliers, const double& huberMultiplier) -> (the return value, `inliers`): the second is the
    reference's out-parameter, which is the OUTLIER share nBad / nInitialCorrespondences (src/cOptimizer.cpp:454-456)."""
    return PoseOptimizationBatch([F], points, huberMultiplier, device, ctx)[0]


# ---------------------------------------------------------------------------------------------- a loop candidate's Sim3 (mcs_sim3_optimize)
class Sim3:
    """g2o::Sim3 as OptimizeSim3 takes and leaves it.  Built from (R, t, s) like the g2o::Sim3 of cLoopClosing::ComputeSim3; after an optimisation q holds the
    quaternion in coeffs() order (x, y, z, w; not normalised, as in the reference), R its toRotationMatrix(), t and s the rest."""

    def __init__(self, R, t, s):
        self.R, self.t, self.s = np.asarray(R, np.float64).reshape(3, 3).copy(), np.asarray(t, np.float64).reshape(3).copy(), float(s)
        self.q = None


def OptimizeSim3Batch(problems, camSystem, device=False, ctx=None, diag=False):
    """cOptimizer::OptimizeSim3 (src/cOptimizerLoopStuff.cpp:58-264) for a list of candidates over one rig (camSystem: M_c and the cameras), as ONE call
    (mcs_sim3_optimize).  problems: dicts with Xw [n][2][3], cam [n][2], obs [n][2][2], w [n][2] (include/mcs_c.h says what each holds), Mt_inv [2][4][4],
    R12, t12, s12 and optionally std_sim (default 4.0, cOptimizer::stdSim).  device=True: every array in device memory, nothing read back before the call has
    returned.  -> a list of dicts: S12 [8] (qx qy qz qw tx ty tz s), R12 [3][3], keep [n] (1 = the match stays), n_inliers; diag=True: (that list, the
    mcs_sim3opt_diag records)"""
    from ._capi import SIM3OPT_DIAG_DTYPE, Sim3OptProblem
    ctx = ctx or default_context()
    npb = len(problems)
    if npb == 0:
        check(lib().mcs_sim3_optimize(ctx.h, 0, None, None, None, 0, None, None, None, None, None, MEM_HOST, None, None, None, None, None))
        return ([], np.zeros(0, SIM3OPT_DIAG_DTYPE)) if diag else []
    mem = _DEVICE if device else _HOST
    nr = camSystem.GetNrCams()
    ocs = (type(camSystem.cams[0].ocam) * nr)(*[cm.ocam for cm in camSystem.cams])
    f8 = lambda k, shape: np.ascontiguousarray([np.asarray(p[k], np.float64).reshape(shape) for p in problems], np.float64)
    g = dict(Mc=np.ascontiguousarray([np.asarray(camSystem.M_c[c], np.float64).reshape(16) for c in range(nr)], np.float64), ocs=np.frombuffer(ocs, np.uint8).copy(),
             Mt=f8("Mt_inv", 32), std=np.array([float(p.get("std_sim", 4.0)) for p in problems], np.float64), R=f8("R12", 9), t=f8("t12", 3),
             s=np.array([float(p["s12"]) for p in problems], np.float64), S=np.zeros((npb, 8)), Ro=np.zeros((npb, 9)), nin=np.zeros(npb, np.int32),
             diag=np.zeros(npb, SIM3OPT_DIAG_DTYPE))
    g = {k: mem.put(v) for k, v in g.items()}
    ns = [len(np.asarray(p["cam"]).reshape(-1, 2)) for p in problems]
    per = [dict(Xw=mem.put(np.ascontiguousarray(p["Xw"], np.float64).reshape(-1)), cam=mem.put(np.ascontiguousarray(p["cam"], np.int32).reshape(-1)),
                obs=mem.put(np.ascontiguousarray(p["obs"], np.float64).reshape(-1)), w=mem.put(np.ascontiguousarray(p["w"], np.float64).reshape(-1)),
                keep=mem.put(np.zeros(max(n, 1), np.uint8))) for p, n in zip(problems, ns)]
    pr = (Sim3OptProblem * npb)(*[Sim3OptProblem(mem.ptr(q["Xw"]) if n else None, mem.ptr(q["cam"]) if n else None, mem.ptr(q["obs"]) if n else None,
                                                 mem.ptr(q["w"]) if n else None, n) for q, n in zip(per, ns)])
    outs = (C.c_void_p * npb)(*[mem.ptr(q["keep"]) for q in per])
    check(lib().mcs_sim3_optimize(ctx.h, npb, pr, mem.ptr(g["Mc"]), mem.ptr(g["ocs"]), nr, mem.ptr(g["Mt"]), mem.ptr(g["std"]), mem.ptr(g["R"]), mem.ptr(g["t"]),
                                  mem.ptr(g["s"]), mem.kind, mem.ptr(g["S"]), mem.ptr(g["Ro"]), outs, mem.ptr(g["nin"]), mem.ptr(g["diag"])))
    # ---- only now the host looks at anything
    S, Ro, nin = (mem.read(g[k]) for k in ("S", "Ro", "nin"))
    res = [dict(S12=S[p].copy(), R12=Ro[p].reshape(3, 3).copy(), keep=mem.read(per[p]["keep"])[:ns[p]].copy(), n_inliers=int(nin[p])) for p in range(npb)]
    return (res, mem.read(g["diag"])) if diag else res


def _sim3_correspondences(pKF1, pKF2, vpMatches1, stdSim):
    """the pointer tests of src/cOptimizerLoopStuff.cpp:117-199 -> (the problem's arrays, the index into vpMatches1 of each correspondence).  Reproduced: e12
    projects with pKF1's camera of feature i2 and e21 with pKF2's camera of feature i (the point vertex an edge holds carries the other side's index), and the
    information of e21 is GetSigma2, not its inverse (:188).  A match that pKF2 does not observe (GetIndexInKeyFrame empty: the reference indexes an empty
    vector) is skipped like i2 < 0; a crossed index beyond the other keyframe's features (the reference dereferences find() == end()) is an IndexError."""
    vp1 = pKF1.GetMapPointMatches()
    Xw, cam, obs, w, at = [], [], [], [], []
    for i, mp2 in enumerate(vpMatches1):
        if mp2 is None:
            continue
        mp1 = vp1[i]
        idx2 = mp2.GetIndexInKeyFrame(pKF2)
        if mp1 is None or not idx2 or mp1.isBad() or mp2.isBad() or idx2[0] < 0:
            continue
        i2 = int(idx2[0])
        k1, k2 = pKF1.GetKeyPoint(i), pKF2.GetKeyPoint(i2)
        Xw.append([np.asarray(mp1.GetWorldPos(), np.float64).reshape(-1)[:3], np.asarray(mp2.GetWorldPos(), np.float64).reshape(-1)[:3]])
        cam.append([int(pKF1.keypoint_to_cam[i2]), int(pKF2.keypoint_to_cam[i])])
        obs.append([[float(k1["x"]), float(k1["y"])], [float(k2["x"]), float(k2["y"])]])
        w.append([float(pKF1.GetInvSigma2(int(k1["octave"]))), float(pKF2.GetSigma2(int(k2["octave"])))])
        at.append(i)
    n = len(at)
    return dict(Xw=np.asarray(Xw, np.float64).reshape(n, 2, 3), cam=np.asarray(cam, np.int32).reshape(n, 2), obs=np.asarray(obs, np.float64).reshape(n, 2, 2),
                w=np.asarray(w, np.float64).reshape(n, 2), Mt_inv=[_inv_mat(pKF1.camSystem.M_t), _inv_mat(pKF2.camSystem.M_t)], std_sim=stdSim), at


def OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, stdSim=4.0, device=False, ctx=None):
    """int cOptimizer::OptimizeSim3(cMultiKeyFrame*, cMultiKeyFrame*, vector<cMapPoint*>& vpMatches1, g2o::Sim3& g2oS12) -> the return value.  vpMatches1 is
    nulled in place (None) where the reference nulls it; g2oS12 (a Sim3 built from R, t, s) gets q, R, t, s of the optimised estimate, and is left as it
    was on the `return 0` path.  stdSim: cOptimizer::stdSim."""
    pr, at = _sim3_correspondences(pKF1, pKF2, vpMatches1, stdSim)
    pr.update(R12=g2oS12.R, t12=g2oS12.t, s12=g2oS12.s)
    res, dg = OptimizeSim3Batch([pr], pKF1.camSystem, device, ctx, diag=True)
    r, d = res[0], dg[0]
    for k, i in zip(r["keep"], at):
        if not k:
            vpMatches1[i] = None
    if d["status"] == 0 and d["n_corr"] - d["n_bad1"] >= 3:   # not the return-0 path (:234-235): g2oS12 = vSim3_recov->estimate() (:260-261)
        g2oS12.q, g2oS12.R, g2oS12.t, g2oS12.s = r["S12"][:4].copy(), r["R12"], r["S12"][4:7].copy(), float(r["S12"][7])
    return r["n_inliers"]


# ---------------------------------------------------------------------------------------------- local bundle adjustment (mcs_local_bundle_adjustment)
def LocalBundleAdjustmentArrays(kf_pose, kf_fixed, n_local, pos, pt_first, edge_kf, edge_cam, edge_key, Mc_min, cams, inv_sigma2, std_recon=2.0, total_obs=None,
                                bad_obs=None, stop_flag=None, device=False, ctx=None, with_t=True):
    """mcs_local_bundle_adjustment over arrays (include/mcs_c.h says what each holds).  cams: camera dicts or Ocam structs.  stop_flag: None (pbStopFlag ==
    NULL: the call that optimises), a bool, or a one-element list that is read and written in place like the reference's bool*.  device=True: every array in
    device memory.  -> dict: status, kf_pose [n_kfs][6], kf_t [n_local][3], pos, edge_state, pt_state, diag (an LBA_DIAG_DTYPE record), stop_flag (its value
    on return, None without one), arrays (the call's arrays where they live: DeviceArray objects in device kind, for a chain without a host visit)"""
    from ._capi import LBA_DIAG_DTYPE, LbaDiag, Ocam
    ctx = ctx or default_context()
    mem = _DEVICE if device else _HOST
    kf_pose = np.ascontiguousarray(kf_pose, np.float64).reshape(-1, 6)
    pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
    nk, P, E, nr = len(kf_pose), len(pos), len(edge_kf), len(cams)
    ocs = (Ocam * max(nr, 1))(*[c if isinstance(c, Ocam) else make_ocam(c) for c in cams])
    sig = np.ascontiguousarray(inv_sigma2, np.float64)
    i4 = lambda a, n: None if a is None else np.ascontiguousarray(a, np.int32).reshape(n)
    g = dict(pose=kf_pose.copy(), fixed=np.ascontiguousarray(kf_fixed, np.uint8).reshape(nk), t=np.zeros((max(n_local, 1), 3)) if with_t else None, pos=pos.copy(),
             first=i4(pt_first, P + 1), ekf=i4(edge_kf, E), ecam=i4(edge_cam, E), key=np.ascontiguousarray(edge_key, KP_DTYPE).reshape(E), total=i4(total_obs, P),
             bad=i4(bad_obs, P), Mc=np.ascontiguousarray(Mc_min, np.float64).reshape(nr, 6), ocs=np.frombuffer(ocs, np.uint8).copy(), sig=sig,
             estate=np.zeros(max(E, 1), np.uint8), pstate=np.full(max(P, 1), 1, np.uint8))
    g = {k: mem.put(v) for k, v in g.items()}
    flag = None if stop_flag is None else C.c_int32(int(bool(stop_flag[0] if isinstance(stop_flag, list) else stop_flag)))
    dg = LbaDiag()
    check(lib().mcs_local_bundle_adjustment(ctx.h, nk, int(n_local), mem.ptr(g["pose"]), mem.ptr(g["fixed"]), mem.ptr(g["t"]), P, mem.ptr(g["pos"]), mem.ptr(g["first"]),
                                            E, mem.ptr(g["ekf"]), mem.ptr(g["ecam"]), mem.ptr(g["key"]), mem.ptr(g["total"]), mem.ptr(g["bad"]), mem.ptr(g["Mc"]),
                                            mem.ptr(g["ocs"]), nr, mem.ptr(g["sig"]), len(sig), float(std_recon), None if flag is None else C.byref(flag), mem.kind,
                                            mem.ptr(g["estate"]), mem.ptr(g["pstate"]), C.byref(dg)))
    if isinstance(stop_flag, list):
        stop_flag[0] = bool(flag.value)
    diag = np.frombuffer(bytes(dg), LBA_DIAG_DTYPE)[0]
    return dict(status=int(diag["status"]), kf_pose=mem.read(g["pose"]), kf_t=mem.read(g["t"])[:n_local] if with_t else None, pos=mem.read(g["pos"]),
                edge_state=mem.read(g["estate"])[:E], pt_state=mem.read(g["pstate"])[:P], diag=diag, stop_flag=None if flag is None else bool(flag.value), arrays=g)


def _observations(mp):
    """{keyframe: [feature, ...]} of a map point as std::map<cMultiKeyFrame*, ...> iterates it: ascending mnId (the project's convention)"""
    obs = mp.GetObservations() if hasattr(mp, "GetObservations") else mp.mObservations
    items = obs.items() if hasattr(obs, "items") else obs
    return sorted(((k, list(v)) for k, v in items), key=lambda kv: kv[0].mnId)


def _lba_lists(pKF):
    """lLocalKeyFrames, lLocalMapPoints, lFixedCameras and the fixed flags of src/cOptimizer.cpp:473-529, 555-595.  Reproduced: mnBALocalForKF is set on bad
    neighbours too (:484), so a bad neighbour never becomes a fixed camera; oneFixed is overwritten per keyframe (:564) and so reflects the LAST local keyframe,
    keyframe 0 is fixed wherever it stands, and the fallback (:575-581) fixes the first local keyframe as well unless keyframe 0 stood last or a fixed camera
    exists."""
    bad = lambda k: hasattr(k, "isBad") and k.isBad()
    neigh = list(pKF.GetVectorCovisibleKeyFrames() if hasattr(pKF, "GetVectorCovisibleKeyFrames") else pKF.mvpOrderedConnectedKeyFrames)
    local = [pKF] + [k for k in neigh if not bad(k)]
    marked = {id(k) for k in [pKF] + neigh}
    points, seen = [], set()
    for k in local:
        for mp in k.GetMapPointMatches():
            if _good(mp) and id(mp) not in seen:
                seen.add(id(mp))
                points.append(mp)
    fixed = []
    for mp in points:
        for k, _ in _observations(mp):
            if id(k) not in marked:
                marked.add(id(k))                        # mnBAFixedForKF is set before the isBad test (:524-526)
                if not bad(k):
                    fixed.append(k)
    is_fixed = np.ones(len(local) + len(fixed), np.uint8)
    one_fixed = False
    for i, k in enumerate(local):
        one_fixed = k.mnId == 0
        is_fixed[i] = one_fixed
    if not one_fixed and not fixed:
        is_fixed[0] = 1
    return local, points, fixed, is_fixed


def LocalBundleAdjustment(pKF, pbStopFlag=None, device=False, store=None, ctx=None, stdRecon=2.0):
    """std::list<cMultiKeyFrame*> cOptimizer::LocalBundleAdjustment(pKF, pMap, nrIters, getCovMats, pbStopFlag) (src/cOptimizer.cpp:461-874) -> lLocalKeyFrames.
    Keyframes: mnId, isBad(), GetVectorCovisibleKeyFrames() (or mvpOrderedConnectedKeyFrames), GetMapPointMatches(), camSystem (GetPoseMin, Get_M_c_min,
    Set_M_t_from_min), keypoint_to_cam, GetKeyPoint, mvInvLevelSigma2, and EraseMapPointMatch(idx) where they have it (else mvpMapPoints[idx] = None).  Points:
    isBad(), GetWorldPos(), GetObservations() (or mObservations), and SetWorldPos / EraseObservation / SetBadFlag where they have them (else mWorldPos /
    mObservations / mbBad are set).  pbStopFlag: None or a one-element list, as the reference's bool*: NULL is the call that optimises — with a flag, g2o's
    terminate action writes it when round one converges, and the reference then writes nothing back (:756-762).
    store: a cCovisibility; the call then ends with SetPose of the local keyframes and UpdateMapPoints of the written points (:866-867), which need mpRefKF on
    the points and mvScaleFactors on pKF."""
    local, points, fixed, is_fixed = _lba_lists(pKF)
    if len(local) <= 1:                                   # :489
        return []
    kfs = local + fixed
    slot = {id(k): i for i, k in enumerate(kfs)}
    bad = lambda k: hasattr(k, "isBad") and k.isBad()
    first, ekf, ecam, keys, at, total, badobs = [0], [], [], [], [], [], []
    for mp in points:
        t = b = 0
        for k, feats in _observations(mp):
            t += len(feats)
            if bad(k):
                b += len(feats)
                continue
            for i in feats:
                ekf.append(slot[id(k)])
                ecam.append(int(k.keypoint_to_cam[i]))
                keys.append(k.GetKeyPoint(i))
                at.append((k, int(i)))
        first.append(len(ekf))
        total.append(t)
        badobs.append(b)
    rig = pKF.camSystem
    nr = rig.GetNrCams()
    key = np.zeros(len(keys), KP_DTYPE)
    for j, kp in enumerate(keys):
        key[j]["x"], key[j]["y"], key[j]["octave"] = kp["x"], kp["y"], kp["octave"]
    r = LocalBundleAdjustmentArrays([k.camSystem.GetPoseMin() for k in kfs], is_fixed, len(local), [np.asarray(mp.GetWorldPos(), np.float64).reshape(-1)[:3] for mp in points],
                                    first, ekf, ecam, key, [rig.Get_M_c_min(c) for c in range(nr)], [cm.ocam for cm in rig.cams], pKF.mvInvLevelSigma2, stdRecon,
                                    total_obs=total, bad_obs=badobs, stop_flag=pbStopFlag, device=device, ctx=ctx)
    pt_of = np.repeat(np.arange(len(points)), np.diff(first))
    for e in np.nonzero(r["edge_state"])[0]:              # EraseMapPointMatch + EraseObservation (:777-778, :810-811)
        k, i = at[e]
        mp = points[pt_of[e]]
        if hasattr(k, "EraseMapPointMatch"):
            k.EraseMapPointMatch(i)
        else:
            k.mvpMapPoints[i] = None
        if hasattr(mp, "EraseObservation"):
            mp.EraseObservation(k, i)
        else:
            for kf, lst in (mp.mObservations.items() if hasattr(mp.mObservations, "items") else mp.mObservations):
                if kf is k and i in lst:
                    lst.remove(i)
    written = []
    for p, mp in enumerate(points):
        if r["pt_state"][p] == 2:
            mp.SetBadFlag() if hasattr(mp, "SetBadFlag") else setattr(mp, "mbBad", True)
        elif r["pt_state"][p] == 0:
            mp.SetWorldPos(r["pos"][p].copy()) if hasattr(mp, "SetWorldPos") else setattr(mp, "mWorldPos", r["pos"][p].copy())
            written.append(p)
    if r["status"] == 0:
        for i, k in enumerate(local):
            if not bad(k):
                k.camSystem.Set_M_t_from_min(r["kf_pose"][i])
        if store is not None:
            store.SetPose(local, ts=r["kf_t"])
            if written and all(hasattr(points[p], "mpRefKF") for p in written):
                store.UpdateMapPoints([points[p] for p in written], r["pos"][written], [points[p].mpRefKF for p in written], pKF.mvScaleFactors)
    return local


# ---------------------------------------------------------------------------------------------- the essential graph (mcs_optimize_essential_graph)
def OptimizeEssentialGraphArrays(Scw, Snc, has_nc, kf_fixed, edge_i, edge_j, edge_kind, pos, pt_ref, device=False, ctx=None, with_t=True):
    """mcs_optimize_essential_graph over arrays (include/mcs_c.h says what each holds).  device=True: every array in device memory.  -> dict: status, Scw_out
    [n_kfs][8], pose [n_kfs][16], kf_t [n_kfs][3], pos, diag (an EG_DIAG_DTYPE record), arrays (the call's arrays where they live: DeviceArray objects in
    device kind, for a chain without a host visit)"""
    from ._capi import EG_DIAG_DTYPE, EgDiag
    ctx = ctx or default_context()
    mem = _DEVICE if device else _HOST
    Scw = np.ascontiguousarray(Scw, np.float64).reshape(-1, 8)
    pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
    K, E, P = len(Scw), len(edge_i), len(pos)
    g = dict(Scw=Scw, Snc=np.ascontiguousarray(Snc, np.float64).reshape(K, 8), has_nc=np.ascontiguousarray(has_nc, np.uint8).reshape(K),
             fixed=np.ascontiguousarray(kf_fixed, np.uint8).reshape(K), ei=np.ascontiguousarray(edge_i, np.int32).reshape(E),
             ej=np.ascontiguousarray(edge_j, np.int32).reshape(E), kind=np.ascontiguousarray(edge_kind, np.uint8).reshape(E), pos=pos.copy(),
             ref=np.ascontiguousarray(pt_ref, np.int32).reshape(P), out=np.zeros((max(K, 1), 8)), pose=np.zeros((max(K, 1), 16)),
             t=np.zeros((max(K, 1), 3)) if with_t else None)
    g = {k: mem.put(v) for k, v in g.items()}
    dg = EgDiag()
    check(lib().mcs_optimize_essential_graph(ctx.h, K, mem.ptr(g["Scw"]), mem.ptr(g["Snc"]), mem.ptr(g["has_nc"]), mem.ptr(g["fixed"]), E, mem.ptr(g["ei"]),
                                             mem.ptr(g["ej"]), mem.ptr(g["kind"]), P, mem.ptr(g["pos"]), mem.ptr(g["ref"]), mem.kind, mem.ptr(g["out"]),
                                             mem.ptr(g["pose"]), mem.ptr(g["t"]), C.byref(dg)))
    diag = np.frombuffer(bytes(dg), EG_DIAG_DTYPE)[0]
    return dict(status=int(diag["status"]), Scw_out=mem.read(g["out"])[:K], pose=mem.read(g["pose"])[:K], kf_t=mem.read(g["t"])[:K] if with_t else None,
                pos=mem.read(g["pos"]), diag=diag, arrays=g)


def _quat_from_rotation(R):
    """Eigen's Quaternion(const Matrix3d&) (Geometry/Quaternion.h:720-759, Shoemake) as Sim3(R, t, 1.0) runs it and csrc/mcs_sim3g.h restates it: x y z w"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = float(R[0, 0]) + (float(R[1, 1]) + float(R[2, 2]))
    q = [0.0] * 4
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (float(R[2, 1]) - float(R[1, 2])) * t, (float(R[0, 2]) - float(R[2, 0])) * t, (float(R[1, 0]) - float(R[0, 1])) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        v = float(R[i, i]) - float(R[j, j]) - float(R[k, k]) + 1.0
        t = math.sqrt(v) if v >= 0 else math.nan
        q[i] = 0.5 * t
        t = float(np.float64(0.5) / np.float64(t))
        q[3] = (float(R[k, j]) - float(R[j, k])) * t
        q[j] = (float(R[j, i]) + float(R[i, j])) * t
        q[k] = (float(R[k, i]) + float(R[i, k])) * t
    return q


def _sim3_row(S):
    """qx qy qz qw tx ty tz s of a KeyFrameAndPose entry: eight numbers as they are, or a Sim3 (its q where an optimisation left one, else the conversion of R)"""
    if isinstance(S, Sim3):
        return list(S.q if S.q is not None else _quat_from_rotation(S.R)) + [float(v) for v in S.t] + [float(S.s)]
    return [float(v) for v in np.asarray(S, np.float64).reshape(8)]


def _essential_graph_lists(pMap, pLoopMKF, pCurMKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, minNumFeat=100):
    """The vertices, edges and point references of src/cOptimizerLoopStuff.cpp:291-464, 490-501 -> (kfs, points, arrays).  Keyframes and the entries of
    LoopConnections are taken in ascending mnId (the project's convention where the reference iterates a container ordered by address).  A bad keyframe gets
    no vertex; an edge that names one is left out (the reference hands g2o a null vertex there, which its addEdge dereferences)."""
    bad = lambda k: hasattr(k, "isBad") and k.isBad()
    by_id = lambda ks: sorted(ks, key=lambda k: k.mnId)
    kfs = [k for k in by_id(pMap.GetAllKeyFrames()) if not bad(k)]
    slot = {id(k): i for i, k in enumerate(kfs)}
    find = lambda table, k: next((v for kk, v in (table.items() if hasattr(table, "items") else table) if kk is k), None)
    Scw, Snc, has_nc = [], [], []
    for k in kfs:
        c = find(CorrectedSim3, k)
        if c is not None:
            Scw.append(_sim3_row(c))
        else:
            Minv = np.asarray(k.GetPoseInverse(), np.float64).reshape(4, 4)
            Scw.append(_quat_from_rotation(Minv[:3, :3]) + [float(v) for v in Minv[:3, 3]] + [1.0])
        n = find(NonCorrectedSim3, k)
        Snc.append(_sim3_row(n) if n is not None else [0.0] * 8)
        has_nc.append(0 if n is None else 1)
    ei, ej, kind = [], [], []
    items = LoopConnections.items() if hasattr(LoopConnections, "items") else LoopConnections
    for k, conns in sorted(items, key=lambda kv: kv[0].mnId):
        for c in by_id(conns):
            if (k.mnId != pCurMKF.mnId or c.mnId != pLoopMKF.mnId) and k.GetWeight(c) < minNumFeat:
                continue
            if id(k) in slot and id(c) in slot:
                ei.append(slot[id(k)]), ej.append(slot[id(c)]), kind.append(0)
    for k in kfs:
        others = []
        parent = k.GetParent()
        if parent is not None:
            others.append(parent)
        others += [l for l in by_id(k.GetLoopEdges()) if l.mnId < k.mnId]
        others += [c for c in k.GetCovisiblesByWeight(minNumFeat) if c.mnId < k.mnId]
        for o in others:
            if id(o) in slot:
                ei.append(slot[id(k)]), ej.append(slot[id(o)]), kind.append(1)
    points = [mp for mp in pMap.GetAllMapPoints() if not (hasattr(mp, "isBad") and mp.isBad())]
    ref = []
    for mp in points:
        if getattr(mp, "mnCorrectedByKF", -1) == pCurMKF.mnId:
            ref.append(next((i for i, k in enumerate(kfs) if k.mnId == mp.mnCorrectedReference), -1))
        else:
            r = mp.GetReferenceKeyFrame() if hasattr(mp, "GetReferenceKeyFrame") else mp.mpRefKF
            ref.append(slot.get(id(r), -1))
    fixed = [1 if k is pLoopMKF else 0 for k in kfs]
    pos = [np.asarray(mp.GetWorldPos(), np.float64).reshape(-1)[:3] for mp in points]
    return kfs, points, (Scw, Snc, has_nc, fixed, ei, ej, kind, np.asarray(pos, np.float64).reshape(-1, 3), ref)


def OptimizeEssentialGraph(pMap, pLoopMKF, pCurMKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, device=False, store=None, ctx=None):
    """void cOptimizer::OptimizeEssentialGraph(pMap, pLoopMKF, pCurMKF, Scurw, NonCorrectedSim3, CorrectedSim3, LoopConnections)
    (src/cOptimizerLoopStuff.cpp:267-513) -> the result of OptimizeEssentialGraphArrays.  pMap: GetAllKeyFrames(), GetAllMapPoints().  Keyframes: mnId, isBad(),
    GetPoseInverse(), GetParent(), GetLoopEdges(), GetCovisiblesByWeight(w), GetWeight(kf), SetPose(M).  Points: isBad(), GetWorldPos(), SetWorldPos(X),
    mnCorrectedByKF, mnCorrectedReference, GetReferenceKeyFrame() (or mpRefKF).  The two KeyFrameAndPose tables: {keyframe: Sim3 or eight numbers qx qy qz qw
    tx ty tz s}.  LoopConnections: {keyframe: keyframes}.  A point whose reference keyframe has no vertex is left as it is.
    store: a cCovisibility; the call then ends with SetPose of the keyframes and UpdateMapPoints of the moved points (UpdateNormalAndDepth, :511), which need
    mpRefKF on the points and mvScaleFactors on pCurMKF; what UpdateMapPoints returns is the result's "update", the points it was given "updated".  The
    wrapper hands the store the HOST copies of kf_t and pos it has read back for SetPose / SetWorldPos anyway; the chain without a host visit is the C
    calls' (the result's "arrays" hold the device arrays of a device-kind call)."""
    kfs, points, arrays = _essential_graph_lists(pMap, pLoopMKF, pCurMKF, NonCorrectedSim3, CorrectedSim3, LoopConnections)
    r = OptimizeEssentialGraphArrays(*arrays, device=device, ctx=ctx)
    if r["status"] != 0:
        return r
    for i, k in enumerate(kfs):
        k.SetPose(r["pose"][i].reshape(4, 4).copy())
    moved = [p for p in range(len(points)) if arrays[8][p] >= 0]
    for p in moved:
        mp = points[p]
        mp.SetWorldPos(r["pos"][p].copy()) if hasattr(mp, "SetWorldPos") else setattr(mp, "mWorldPos", r["pos"][p].copy())
    if store is not None:
        store.SetPose(kfs, ts=r["kf_t"])
        if moved and all(hasattr(points[p], "mpRefKF") for p in moved):
            r["updated"] = [points[p] for p in moved]
            r["update"] = store.UpdateMapPoints(r["updated"], r["pos"][moved], [points[p].mpRefKF for p in moved], pCurMKF.mvScaleFactors)
    return r
