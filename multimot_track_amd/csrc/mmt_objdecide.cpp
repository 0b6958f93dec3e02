// multimot_track_amd/csrc/mmt_objdecide.cpp -- B7 decisions and B8 label association on the host
// (mmt_objdecide.h).

#include "mmt_objdecide.h"

#include <algorithm>

namespace mmt {

ObjDecision obj_decide(const LabelStats* stats, const int* hist, bool bSecond,
                       const std::vector<int>& lastModLabel,
                       const std::vector<int>& lastSemPosition) {
  ObjDecision D;
  // ---- B7 decisions (Tracking.cc:1424-1536); labels ascending = UniLab order
  std::vector<int>& objLabelsNew = D.labels;  // semantic label of each kept object
  for (int l = 1; l < kMaxLabel; l++) {
    const LabelStats& s = stats[l];
    if (s.cnt == 0) continue;
    const float count = (float)s.bcnt;
    if (count / s.cnt > 0.5f) continue;  // mostly on the image boundary
    if (!(s.cnt > 100)) continue;        // fewer than 100 points
    const float sf_count = (float)s.sfcnt;
    if (sf_count / s.cnt > 0.3f) continue;            // static object
    if (s.depth_sum / s.cnt > 25.0) continue;         // too far
    objLabelsNew.push_back(l);
  }
  // ---- B8 label association (Tracking.cc:1556-1630)
  int mx;
  if (bSecond)
    mx = 1;
  else if (!lastModLabel.empty())
    mx = *std::max_element(lastModLabel.begin(), lastModLabel.end()) + 1;
  else
    mx = 1;  // uninitialised in the reference (Tracking.cc:1557): pinned 1
  const int nobj = (int)objLabelsNew.size();
  std::vector<int>& LabId = D.LabId;
  LabId.resize(nobj);
  for (int i = 0; i < nobj; i++) {
    const int l = objLabelsNew[i];
    int New_lab = 0, best = -1;
    for (int ll = 0; ll < kMaxLabel; ll++) {  // std::map order: ascending last label
      const int c = hist[l * kMaxLabel + ll];
      if (c > best && c > 0) {
        best = c;
        New_lab = ll;
      }
    }
    if (bSecond) {
      LabId[i] = mx++;
    } else {
      bool exist = false;
      for (size_t k = 0; k < lastSemPosition.size() && k < lastModLabel.size(); k++)
        if (lastSemPosition[k] == New_lab) {
          LabId[i] = lastModLabel[k];
          exist = true;
          break;
        }
      if (!exist) LabId[i] = mx++;
    }
  }
  return D;
}

}  // namespace mmt
