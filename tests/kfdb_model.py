"""Line-by-line Python statement of cMultiKeyFrameDatabase (src/cMultiKeyFrameDatabase.cpp), DBoW2 L1Scoring::score
(ThirdParty/DBoW2/DBoW2/ScoringObject.cpp:23-66) and the BowVector build of TemplatedVocabulary::transform (TF_IDF branch,
ThirdParty/DBoW2/DBoW2/TemplatedVocabulary.h:1147-1163) + BowVector::normalize(L1).  The model the device keyframe database is checked
against, bit for bit.

Keyframes are plain objects with the reference's per-keyframe state (include/cMultiKeyFrame.h): mnRelocQuery / mnRelocWords / mRelocScore,
mnLoopQuery / mnLoopWords / mLoopScore.  Only the two query ids are initialised by the reference (src/cMultiKeyFrame.cpp:44-45); the
counters start at 0 here, and a score never written reads 0.0 (the reference reads an unwritten double: DESIGN.md section 7, trap (a)).
Python floats are IEEE doubles and every operation below is written in the reference's order, so the doubles are the reference's."""


class KF:
    """The parts of cMultiKeyFrame the database touches.  bow: [(word id, value)] in ascending word id (the std::map mBowVec)."""

    def __init__(self, mnId, bow, neighbours=()):
        self.mnId = int(mnId)
        self.bow = [(int(w), float(v)) for w, v in bow]
        self.neighbours = list(neighbours)   # ordered covisibles: GetBestCovisibilityKeyFrames(10) takes the first <= 10
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = 0.0
        self.mnLoopQuery = 0
        self.mnLoopWords = 0
        self.mLoopScore = 0.0

    def GetBestCovisibilityKeyFrames(self, n):   # src/cMultiKeyFrame.cpp:231-240
        return self.neighbours[:n]


def l1_score(v1, v2):
    """L1Scoring::score(v1, v2): ScoringObject.cpp:32-66.  vi from v1."""
    i = j = 0
    score = 0.0
    while i < len(v1) and j < len(v2):
        (a, vi), (b, wi) = v1[i], v2[j]
        if a == b:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif a < b:
            i += 1            # v1.lower_bound(v2_it->first): the next shared word is reached either way
        else:
            j += 1
    return -score / 2.0


def bow_vector(word_of_leaf, weight_of_leaf):
    """TemplatedVocabulary::transform (TF_IDF, L1 scoring => mustNormalize): per feature in order, addWeight(word, weight) when weight > 0
    (:1147-1163), then BowVector::normalize(L1): norm = sum |v| in ascending word order, v /= norm if norm > 0."""
    bow = {}
    for wid, w in zip(word_of_leaf, weight_of_leaf):
        w = float(w)
        if w > 0:
            wid = int(wid)
            if wid in bow:
                bow[wid] += w            # BowVector::addWeight: vit->second += v
            else:
                bow[wid] = w             # insert(vit, value_type(id, v))
    items = sorted(bow.items())
    norm = 0.0
    for _, v in items:
        norm += abs(v)
    if norm > 0.0:
        items = [(k, v / norm) for k, v in items]
    return items


class Database:
    """cMultiKeyFrameDatabase.  mvInvertedFile[word] = list of keyframes (std::list, push_back order)."""

    def __init__(self, n_words):
        self.n_words = n_words
        self.inv = [[] for _ in range(n_words)]

    def add(self, kf):                                   # :43-51
        for w, _ in kf.bow:
            self.inv[w].append(kf)

    def erase(self, kf):                                 # :53-73: the first occurrence in each of its words' lists
        for w, _ in kf.bow:
            lst = self.inv[w]
            for i, x in enumerate(lst):
                if x is kf:
                    del lst[i]
                    break

    def clear(self):                                     # :75-79
        self.inv = [[] for _ in range(self.n_words)]

    def DetectRelocalisationCandidates(self, mnId, bow, trace=None):   # :213-329
        shared = []
        for w, _ in bow:                                 # :224-241
            for kfi in self.inv[w]:
                if kfi.mnRelocQuery != mnId:
                    kfi.mnRelocWords = 0
                    kfi.mnRelocQuery = mnId
                    shared.append(kfi)
                kfi.mnRelocWords += 1
        if not shared:
            return []
        maxCommonWords = 0                               # :246-254
        for kfi in shared:
            if kfi.mnRelocWords > maxCommonWords:
                maxCommonWords = kfi.mnRelocWords
        minCommonWords = int(maxCommonWords * 0.8)       # static_cast<int>: truncation
        scored = []
        for kfi in shared:                               # :262-275
            if kfi.mnRelocWords > minCommonWords:
                si = l1_score(bow, kfi.bow)
                kfi.mRelocScore = si
                scored.append((si, kfi))
        if not scored:
            return []
        accs = []
        bestAccScore = 0.0                               # :281
        for si, kfi in scored:                           # :284-310
            bestScore = si
            accScore = bestScore
            best = kfi
            for kf2 in kfi.GetBestCovisibilityKeyFrames(10):
                if kf2.mnRelocQuery != mnId:
                    continue
                accScore += kf2.mRelocScore
                if kf2.mRelocScore > bestScore:
                    best = kf2
                    bestScore = kf2.mRelocScore
            accs.append((accScore, best))
            if accScore > bestAccScore:
                bestAccScore = accScore
        if trace is not None:
            trace.extend((kfi.mnId, kfi.mnRelocWords, si, acc, b.mnId) for (si, kfi), (acc, b) in zip(scored, accs))
        return _retain(accs, bestAccScore)

    def DetectLoopCandidates(self, kf, minScore, connected=(), trace=None):   # :82-210; kf: mnId + bow; connected: GetConnectedKeyFrames()
        conn = set(id(c) for c in connected)
        mnId = kf.mnId
        shared = []
        for w, _ in kf.bow:                              # :93-113
            for kfi in self.inv[w]:
                if kfi.mnLoopQuery != mnId:
                    kfi.mnLoopWords = 0
                    if id(kfi) not in conn:
                        kfi.mnLoopQuery = mnId
                        shared.append(kfi)
                kfi.mnLoopWords += 1
        if not shared:
            return []
        maxCommonWords = 0
        for kfi in shared:
            if kfi.mnLoopWords > maxCommonWords:
                maxCommonWords = kfi.mnLoopWords
        minCommonWords = int(float(maxCommonWords) * 0.8)
        scored = []
        for kfi in shared:                               # :131-146
            if kfi.mnLoopWords > minCommonWords:
                si = l1_score(kf.bow, kfi.bow)
                kfi.mLoopScore = si
                if si >= minScore:
                    scored.append((si, kfi))
        if not scored:
            return []
        accs = []
        bestAccScore = minScore                          # :152
        for si, kfi in scored:                           # :155-180
            bestScore = si
            accScore = si
            best = kfi
            for kf2 in kfi.GetBestCovisibilityKeyFrames(10):
                if kf2.mnLoopQuery == mnId and kf2.mnLoopWords > minCommonWords:
                    accScore += kf2.mLoopScore
                    if kf2.mLoopScore > bestScore:
                        best = kf2
                        bestScore = kf2.mLoopScore
            accs.append((accScore, best))
            if accScore > bestAccScore:
                bestAccScore = accScore
        if trace is not None:
            trace.extend((kfi.mnId, kfi.mnLoopWords, si, acc, b.mnId) for (si, kfi), (acc, b) in zip(scored, accs))
        return _retain(accs, bestAccScore)


def _retain(accs, bestAccScore):
    """:183-207 / :312-327: accScore > 0.75 * bestAccScore, in list order, each best keyframe once (first occurrence)."""
    minScoreToRetain = 0.75 * bestAccScore
    seen, out = set(), []
    for acc, kfi in accs:
        if acc > minScoreToRetain and id(kfi) not in seen:
            seen.add(id(kfi))
            out.append(kfi)
    return out
