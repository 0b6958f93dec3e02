"""A Python restatement of KeyFrameDatabase::DetectLoopCandidates (KeyFrameDatabase.cc:76-197) and
LoopClosing::DetectLoop (LoopClosing.cc:105-231), written from the reference's text, in two forms:

  literal=True   the inverted file (a list of keyframes per word, in insertion order) and the three
                 per-keyframe scratch fields mnLoopQuery / mnLoopWords / mLoopScore, line by line;
  literal=False  the flat form: per stored keyframe the triple (common, first, sum) from a merge of
                 the two vectors, lKFsSharingWords = the members with common > 0 that are not
                 connected, sorted by (first, add sequence).

One departure, stated by the library too: no per-query state survives a query (the reference's
mnLoopQuery is keyed by the query's id, which it never queries twice), so the scratch fields are
fresh per call.  Scores are DBoW2's L1 / L2 (Vocabulary::score), summed sequentially in Python
floats (doubles); every float of the reference is a numpy float32.

A graph is dict(ordered=[ids per keyframe id], conn=[ids per keyframe id], bad=[0/1 per id]).
"""
import math

import numpy as np

INT_MAX = 2 ** 31 - 1
F = np.float32


def term(vi, wi, scoring):
    if scoring == 1:
        return vi * wi
    return math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)


def common_terms(qw, qv, kw, kv, scoring):
    """[(stored index, query index, term)] over the common words, ascending."""
    pos = {int(w): i for i, w in enumerate(qw)}
    out = []
    for j, w in enumerate(kw):
        i = pos.get(int(w))
        if i is not None:
            out.append((j, i, term(float(qv[i]), float(kv[j]), scoring)))
    return out


def triple(qw, qv, kw, kv, scoring):
    """(common, first, sum): what the kernel writes for one stored vector."""
    t = common_terms(qw, qv, kw, kv, scoring)
    s = 0.0
    for _, _, x in t:
        s += x
    return len(t), (t[0][1] if t else INT_MAX), s


def finish(s, scoring):
    if scoring == 1:
        return 1.0 if s >= 1 else 1.0 - math.sqrt(1.0 - s)
    return -s / 2.0


# ---- the sequential sum and three other orders of the same terms
def sum_sequential(terms):
    s = 0.0
    for x in terms:
        s += x
    return s


def sum_reversed(terms):
    return sum_sequential(list(terms)[::-1])


def sum_pairwise(terms):
    t = list(terms)
    if not t:
        return 0.0
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


def sum_lane_strided(stored_index_and_term):
    """64 partial sums, term of stored index j into lane j % 64, the lanes added at the end."""
    part = [0.0] * 64
    for j, x in stored_index_and_term:
        part[j % 64] += x
    return sum_sequential(part)


class RefLoop:
    def __init__(self, scoring=0, literal=False):
        self.scoring = scoring
        self.literal = literal
        self.vec = {}        # id -> (words, values), in set_bow order
        self.inv = {}        # literal: word -> [ids] in insertion order
        self.members = []    # flat: ids in add order
        self.groups = []     # mvConsistentGroups: [(sorted ids, counter)]
        self.trace = {}      # what the last candidates() call dropped where (for the tests)

    # -- store and database
    def set_bow(self, kf, words, values):
        assert kf not in self.vec
        self.vec[kf] = (np.asarray(words, np.uint32), np.asarray(values, np.float64))

    def is_member(self, kf):
        return kf in self.members

    def db_add(self, kf):
        assert kf in self.vec and kf not in self.members
        self.members.append(kf)
        for w in self.vec[kf][0]:
            self.inv.setdefault(int(w), []).append(kf)

    def db_erase(self, kf):
        if kf not in self.members:
            return
        self.members.remove(kf)
        for w in self.vec[kf][0]:
            self.inv[int(w)].remove(kf)

    def triple(self, q, k):
        return triple(*self.vec[q], *self.vec[k], self.scoring)

    def score(self, q, k):
        return finish(self.triple(q, k)[2], self.scoring)

    # -- KeyFrameDatabase::DetectLoopCandidates
    def candidates(self, kf, min_score, graph):
        min_score = F(min_score)
        connected = set(graph["conn"][kf])
        tr = self.trace = dict(sharing=[], words_dropped=[], score_dropped=[], cut_dropped=[],
                               duplicates=[], first={})
        if self.literal:
            query, nwords, sharing = set(), {}, []
            for w in self.vec[kf][0]:
                for i in self.inv.get(int(w), []):
                    if i not in query:                  # pKFi->mnLoopQuery != pKF->mnId
                        nwords[i] = 0                   # pKFi->mnLoopWords = 0
                        if i not in connected:
                            query.add(i)                # pKFi->mnLoopQuery = pKF->mnId
                            sharing.append(i)
                    nwords[i] += 1
        else:
            t = {i: self.triple(kf, i) for i in self.members}
            sharing = [i for i in self.members if t[i][0] > 0 and i not in connected]
            seq = {i: n for n, i in enumerate(self.members)}
            sharing.sort(key=lambda i: (t[i][1], seq[i]))
            query = set(sharing)
            nwords = {i: t[i][0] for i in sharing}
            tr["first"] = {i: t[i][1] for i in sharing}
        tr["sharing"] = list(sharing)
        if not sharing:
            return []
        max_common = 0
        for i in sharing:
            if nwords[i] > max_common:
                max_common = nwords[i]
        min_common = int(F(max_common) * F(0.8))
        loop_score, scored = {}, []
        for i in sharing:
            if nwords[i] > min_common:
                si = F(self.score(kf, i))
                loop_score[i] = si
                if si >= min_score:
                    scored.append((si, i))
                else:
                    tr["score_dropped"].append(i)
            else:
                tr["words_dropped"].append(i)
        if not scored:
            return []
        acc_list = []
        best_acc = min_score
        for si, i in scored:
            best_score, acc, best = si, si, i
            for k2 in list(graph["ordered"][i])[:10]:
                if k2 in query and nwords[k2] > min_common:
                    acc = F(acc + loop_score[k2])
                    if loop_score[k2] > best_score:
                        best, best_score = k2, loop_score[k2]
            acc_list.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        retain = F(F(0.75) * best_acc)
        out = []
        for acc, i in acc_list:
            if acc > retain:
                if i not in out:
                    out.append(i)
                else:
                    tr["duplicates"].append(i)
            else:
                tr["cut_dropped"].append(i)
        return out

    # -- LoopClosing::DetectLoop
    def detect_loop(self, kf, last_loop_kf_id, graph, consistency_th=3):
        res = dict(ran=False, min_score=F(1), candidates=[], enough=[], n_groups=len(self.groups),
                   cleared=False, double_match=False)
        if kf < last_loop_kf_id + 10:
            self.db_add(kf)
            return res
        min_score = F(1)
        for k in graph["ordered"][kf]:
            if graph["bad"][k]:
                continue
            score = F(self.score(kf, k))
            if score < min_score:
                min_score = score
        cand = self.candidates(kf, min_score, graph)
        res.update(ran=True, min_score=min_score, candidates=cand)
        if not cand:
            self.db_add(kf)
            res["cleared"] = len(self.groups) > 0
            self.groups = []
            res["n_groups"] = 0
            return res
        enough, current = [], []
        consistent_group = [False] * len(self.groups)
        for c in cand:
            group = set(graph["conn"][c])
            group.add(c)
            enough_consistent = False
            consistent_for_some = False
            nmatched = 0
            for ig, (prev, nprev) in enumerate(self.groups):
                consistent = False
                for m in group:
                    if m in prev:
                        consistent = True
                        consistent_for_some = True
                        break
                if consistent:
                    nmatched += 1
                    ncur = nprev + 1
                    if not consistent_group[ig]:
                        current.append((sorted(group), ncur))
                        consistent_group[ig] = True
                    if ncur >= consistency_th and not enough_consistent:
                        enough.append(c)
                        enough_consistent = True
            if nmatched >= 2:
                res["double_match"] = True
            if not consistent_for_some:
                current.append((sorted(group), 0))
        self.groups = current
        self.db_add(kf)
        res.update(enough=enough, n_groups=len(current))
        return res
