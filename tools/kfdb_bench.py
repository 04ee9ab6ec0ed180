"""Device keyframe database (mcs_kfdb_*): batched relocalisation throughput and single-query latency at 256 / 1 024 / 4 096 / 16 384 keyframes.

Keyframe BowVectors come from synthetic 3 x 754 x 480 multi-frames through the shipped vocabulary (tests/golden/small_orb_omni_voc_9_6.yml.gz):
every keyframe keeps a random 40-90 % of one frame's descriptors (perturbation), so the large sizes reuse a handful of extracted frames.  Queries
are fresh subsets.  A sample of queries is checked against the model of tests/kfdb_model.py (candidates and the scored lists, bit for bit).
Prints one JSON line:  python tools/kfdb_bench.py [--sizes 256,1024,4096,16384] [--batch 64] [--reps 20]"""
import argparse
import gzip
import importlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,4096,16384")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--check", type=int, default=2, help="queries per size checked against the model")
    a = ap.parse_args()
    import kfdb_model as M
    mcs = importlib.import_module("multicol-slam_amd")
    FE = importlib.import_module("multicol-slam_amd.frontend")
    io = importlib.import_module("multicol-slam_amd.io")
    synth = importlib.import_module("multicol-slam_amd.synth")
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "voc.yml")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "small_orb_omni_voc_9_6.yml.gz"), "rb") as s, open(path, "wb") as d:
        shutil.copyfileobj(s, d)
    ctx = mcs.Context(0)
    vd = io.load_vocabulary(path)
    shutil.rmtree(tmp)
    voc = FE.cORBVocabulary(vd, ctx=ctx)
    cams = synth.lafida_cameras()
    rig = FE.cMultiCamSys_([FE.cCamModelGeneral_.from_dict(c, synth.mirror_mask(c)) for c in cams])
    ex = FE.mdBRIEFextractorOct(1000, 1.2, 8, 25, 0, 0, 32, 20, False, 2, True, True, 32, ctx=ctx)
    leaves = []
    for f in range(a.frames):
        F = FE.cMultiFrame(synth.synth_multiframe(f * 7, cams), 0.04 * f, [ex] * 3, voc, rig, f)
        leaves.append(voc.descend(F.all_descriptors(), 4)[0])
    rng = np.random.default_rng(1)

    def bow():
        lf = leaves[int(rng.integers(len(leaves)))]
        sel = np.sort(rng.choice(len(lf), int(len(lf) * rng.uniform(0.4, 0.9)), replace=False))
        return M.bow_vector(vd["word_id"][lf[sel]], vd["weight"][lf[sel]])

    L = mcs.lib()
    res = {"metric": "kfdb_relocalisation", "batch": a.batch, "sizes": {}}
    qid = [10 ** 9]
    for n in [int(x) for x in a.sizes.split(",")]:
        db = FE.cMultiKeyFrameDatabase(voc, ctx=ctx, capacity_hint=n)
        kfs = [bow() for _ in range(n)]
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(b) for b in kfs])
        w = np.array([x for b in kfs for x, _ in b], np.int32)
        v = np.array([y for b in kfs for _, y in b], np.float64)
        ids = np.arange(1, n + 1, dtype=np.int64)
        mcs.check(L.mcs_kfdb_add(db.h, n, ids.ctypes.data, off.ctypes.data, w.ctypes.data, v.ctypes.data, mcs.MEM_HOST))
        nb = np.array([rng.choice(n, 10, replace=False) + 1 for _ in range(n)], np.int64)
        ncov = np.full(n, 10, np.int32)
        mcs.check(L.mcs_kfdb_set_covisibility(db.h, n, ids.ctypes.data, nb.ctypes.data, ncov.ctypes.data))
        queries = [bow() for _ in range(a.batch)]
        qoff = np.zeros(a.batch + 1, np.int32)
        qoff[1:] = np.cumsum([len(b) for b in queries])
        qw = np.array([x for b in queries for x, _ in b], np.int32)
        qv = np.array([y for b in queries for _, y in b], np.float64)
        cap = n
        cnt = np.zeros(a.batch, np.int32)
        out = np.zeros(a.batch * cap, np.int64)

        def run(nq):
            q = np.arange(qid[0], qid[0] + nq, dtype=np.int64)
            qid[0] += nq
            mcs.check(L.mcs_kfdb_detect_relocalisation(db.h, nq, q.ctypes.data, qoff.ctypes.data, qw.ctypes.data, qv.ctypes.data, mcs.MEM_HOST, cap,
                                                       cnt.ctypes.data, out.ctypes.data, None))

        for _ in range(3):
            run(a.batch); run(1)
        tb, t1 = [], []
        for _ in range(a.reps):
            t = time.perf_counter(); run(a.batch); tb.append(time.perf_counter() - t)
            t = time.perf_counter(); run(1); t1.append(time.perf_counter() - t)
        # model check on a fresh database: the first `check` queries, one batch
        mod = M.Database(voc.size())
        mk = {i + 1: M.KF(i + 1, kfs[i]) for i in range(n)}
        for i in range(n):
            mk[i + 1].neighbours = [mk[int(j)] for j in nb[i]]
            mod.add(mk[i + 1])
        chk = FE.cMultiKeyFrameDatabase(voc, ctx=ctx)
        mcs.check(L.mcs_kfdb_add(chk.h, n, ids.ctypes.data, off.ctypes.data, w.ctypes.data, v.ctypes.data, mcs.MEM_HOST))
        mcs.check(L.mcs_kfdb_set_covisibility(chk.h, n, ids.ctypes.data, nb.ctypes.data, ncov.ctypes.data))
        k = min(a.check, a.batch)
        q = np.arange(5, 5 + k, dtype=np.int64)
        mcs.check(L.mcs_kfdb_detect_relocalisation(chk.h, k, q.ctypes.data, qoff.ctypes.data, qw.ctypes.data, qv.ctypes.data, mcs.MEM_HOST, cap,
                                                   cnt.ctypes.data, out.ctypes.data, None))
        ok = all(out[j * cap:j * cap + cnt[j]].tolist() == [x.mnId for x in mod.DetectRelocalisationCandidates(int(q[j]), queries[j])] for j in range(k))
        res["sizes"][str(n)] = {"batch_ms": round(1e3 * float(np.median(tb)), 4), "single_ms": round(1e3 * float(np.median(t1)), 4),
                                "queries_per_s": round(a.batch / float(np.median(tb)), 1), "words_per_kf": round(len(w) / n, 1),
                                "model_check": bool(ok), "checked": k}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
