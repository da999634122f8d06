// KeyFrameDatabase.h — C++ host mirror of ORB_SLAM3::KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) over
// liborbx's orbx_kfdb_*: add / erase / clear / clearMap, DetectRelocalizationCandidates (:742-856) and DetectNBestCandidates
// (:612-740) with the reference's names and argument order.  The BoW vectors live on the device; a query scores every key frame
// there and returns the candidates the reference returns, in its order.  Where the reference takes KeyFrame* / Frame* / Map*, the
// mirror takes what it reads of them: mnId, the map's mnId, mBowVec.
//
// What stays with the caller:
//  - the id <-> pointer maps (KeyFrame::mnId, Map::mnId) -- candidates come back as key-frame ids;
//  - the covisibility graph: hand GetBestCovisibilityKeyFrames(10) of a key frame to SetBestCovisibilityKeyFrames whenever
//    UpdateConnections changes it (the list belongs to the database entry: erase drops it), and GetConnectedKeyFrames() of the
//    query key frame to DetectNBestCandidates;
//  - isBad(): KeyFrame::SetBadFlag erases the key frame (src/KeyFrame.cc:679), so bad key frames are not in the database;
//  - Map::IsBad(): the ids of the bad maps are an argument of DetectNBestCandidates.
#ifndef ORBX_SHIM_KEYFRAMEDATABASE_H
#define ORBX_SHIM_KEYFRAMEDATABASE_H

#include <set>

#include "ORBVocabulary.h"

namespace ORB_SLAM3 {

// what DetectNBestCandidates reads of its KeyFrame* pKF
struct KeyFrameQuery {
  const DBoW2::BowVector* mBowVec = nullptr;
  int mnMapId = 0;                       // pKF->GetMap()->GetId()
  std::set<int> spConnectedKeyFrames;    // pKF->GetConnectedKeyFrames(), as mnId
};

class KeyFrameDatabase {
 public:
  // KeyFrameDatabase(const ORBVocabulary& voc), plus the capacity of the device store: key frames, and words per key frame
  KeyFrameDatabase(const ORBVocabulary& voc, int nMaxKeyFrames, int nMaxWordsPerKeyFrame) {
    if (orbx_kfdb_create(voc.handle(), nMaxKeyFrames, nMaxWordsPerKeyFrame, &h_) != ORBX_OK) fail("KeyFrameDatabase");
  }
  ~KeyFrameDatabase() { orbx_kfdb_destroy(h_); }
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

  // add(KeyFrame* pKF): pKF->mnId, pKF->GetMap()->GetId(), pKF->mBowVec
  void add(int nKFId, int nMapId, const DBoW2::BowVector& mBowVec) {
    flatten(mBowVec);
    if (orbx_kfdb_add(h_, nKFId, nMapId, words_.data(), values_.data(), (int)words_.size()) != ORBX_OK) fail("add");
  }
  // add of image `image` of the extractor's last orbx_bow_transform_batch: the vector never leaves the device
  void add(int nKFId, int nMapId, orbx_extractor* ex, int image) {
    if (orbx_kfdb_add_from_batch(h_, ex, image, nKFId, nMapId) != ORBX_OK) fail("add");
  }
  void erase(int nKFId) {
    if (orbx_kfdb_erase(h_, nKFId) != ORBX_OK) fail("erase");
  }
  void clear() {
    if (orbx_kfdb_clear(h_) != ORBX_OK) fail("clear");
  }
  void clearMap(int nMapId) {
    if (orbx_kfdb_clear_map(h_, nMapId) < 0) fail("clearMap");
  }
  size_t size() const { return (size_t)std::max(orbx_kfdb_size(h_), 0); }

  // pKF->GetBestCovisibilityKeyFrames(10) of key frame nKFId, as mnIds (more than ten are cut)
  void SetBestCovisibilityKeyFrames(int nKFId, const std::vector<int>& vpNeighs) {
    int32_t best[10];
    for (size_t j = 0; j < 10; j++) best[j] = j < vpNeighs.size() ? vpNeighs[j] : -1;
    const int32_t id = nKFId;
    if (orbx_kfdb_set_covisibles(h_, 1, &id, best) != ORBX_OK) fail("SetBestCovisibilityKeyFrames");
  }

  // DetectRelocalizationCandidates(Frame* F, Map* pMap): F->mBowVec, pMap's id
  std::vector<int> DetectRelocalizationCandidates(const DBoW2::BowVector& mBowVec, int nMapId) {
    flatten(mBowVec);
    std::vector<int32_t> cand(std::max<size_t>(size(), 1));
    int32_t n = 0;
    if (orbx_kfdb_detect_relocalization_candidates(h_, words_.data(), values_.data(), (int)words_.size(), nMapId, cand.data(),
                                                   (int)cand.size(), &n, nullptr) != ORBX_OK)
      fail("DetectRelocalizationCandidates");
    return std::vector<int>(cand.begin(), cand.begin() + n);
  }

  // DetectNBestCandidates(KeyFrame* pKF, vector<KeyFrame*>& vpLoopCand, vector<KeyFrame*>& vpMergeCand, int nNumCandidates)
  void DetectNBestCandidates(const KeyFrameQuery& KF, std::vector<int>& vpLoopCand, std::vector<int>& vpMergeCand, int nNumCandidates,
                             const std::set<int>& spBadMaps = std::set<int>()) {
    if (!KF.mBowVec) throw std::invalid_argument("DetectNBestCandidates: no BoW vector");
    flatten(*KF.mBowVec);
    const std::vector<int32_t> conn(KF.spConnectedKeyFrames.begin(), KF.spConnectedKeyFrames.end()), bad(spBadMaps.begin(), spBadMaps.end());
    std::vector<int32_t> loop((size_t)std::max(nNumCandidates, 1)), merge(loop.size());
    int32_t nl = 0, nm = 0;
    if (orbx_kfdb_detect_n_best_candidates(h_, words_.data(), values_.data(), (int)words_.size(), KF.mnMapId, conn.data(), (int)conn.size(),
                                           bad.data(), (int)bad.size(), nNumCandidates, loop.data(), &nl, merge.data(), &nm,
                                           nullptr) != ORBX_OK)
      fail("DetectNBestCandidates");
    vpLoopCand.assign(loop.begin(), loop.begin() + nl);
    vpMergeCand.assign(merge.begin(), merge.begin() + nm);
  }

  orbx_kfdb* handle() const { return h_; }

 private:
  [[noreturn]] static void fail(const char* what) { throw std::runtime_error(std::string("KeyFrameDatabase::") + what + ": " + orbx_last_error()); }
  void flatten(const DBoW2::BowVector& v) {
    words_.clear();
    values_.clear();
    for (const auto& e : v) {
      words_.push_back(e.first);
      values_.push_back(e.second);
    }
  }
  orbx_kfdb* h_ = nullptr;
  std::vector<uint32_t> words_;
  std::vector<double> values_;
};

}  // namespace ORB_SLAM3
#endif
