// Drives ORB_SLAM3::KeyFrameDatabase (csrc/KeyFrameDatabase.h) in the shape of its two call sites: Tracking::Relocalization
// (src/Tracking.cc:3527) and LoopClosing::NewDetectCommonRegions (src/LoopClosing.cc:363-568: DetectNBestCandidates at :517, then
// add of the current key frame).  Inputs are written by tests/test_kfdb_cpp.py.
//   usage: kfdb_like <voc.txt>                      three made-up key frames and one query of each flavour
//          kfdb_like <voc.txt> <scene.raw> <out>    scene: int32 {nKF, mode (0 relocalisation, 1 N-best), query map, nNumCandidates,
//            nConnected, nBadMaps, nQueryWords}; per key frame int32 {id, map, nWords, nCovisibles}, uint32 words, double values,
//            int32 covisibles; then int32 connected ids, int32 bad maps, uint32 query words, double query values.
//          out: int32 n, candidates (relocalisation) or int32 nLoop, loop candidates, int32 nMerge, merge candidates.
// Without a GPU the vocabulary cannot be loaded: exit 3 and "no-device error".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/KeyFrameDatabase.h"

static_assert(sizeof(orbx_kfdb_details) == 8 + 7 * sizeof(void*), "orbx_kfdb_details");

struct Reader {
  std::vector<char> b;
  size_t pos = 0;
  template <class T>
  std::vector<T> take(size_t n) {
    std::vector<T> v(n);
    if (pos + n * sizeof(T) > b.size()) throw std::runtime_error("scene file too short");
    if (n) std::memcpy(v.data(), b.data() + pos, n * sizeof(T));
    pos += n * sizeof(T);
    return v;
  }
};

static DBoW2::BowVector bow(const std::vector<uint32_t>& w, const std::vector<double>& v) {
  DBoW2::BowVector b;
  for (size_t i = 0; i < w.size(); i++) b.insert(b.end(), std::make_pair(w[i], v[i]));
  return b;
}

static void write_list(std::ofstream& o, const std::vector<int>& v) {
  const int32_t n = (int32_t)v.size();
  o.write(reinterpret_cast<const char*>(&n), 4);
  for (int x : v) {
    const int32_t y = x;
    o.write(reinterpret_cast<const char*>(&y), 4);
  }
}

int main(int argc, char** argv) {
  if (argc != 2 && argc != 4) return 2;
  try {
    ORB_SLAM3::ORBVocabulary voc;
    if (!voc.loadFromTextFile(argv[1])) throw std::runtime_error(orbx_last_error());
    if (argc == 2) {
      ORB_SLAM3::KeyFrameDatabase db(voc, 8, 16);
      const DBoW2::BowVector a = bow({0, 1}, {0.5, 0.5}), b = bow({1}, {1.0});
      db.add(1, 0, a);
      db.add(2, 0, b);
      db.add(3, 1, a);
      db.SetBestCovisibilityKeyFrames(1, {2, 3});
      // Relocalization is performed when tracking is lost: query the KeyFrame Database for keyframe candidates
      std::vector<int> vpCandidateKFs = db.DetectRelocalizationCandidates(a, 0);
      ORB_SLAM3::KeyFrameQuery current;
      current.mBowVec = &a;
      current.spConnectedKeyFrames = {2};
      std::vector<int> vpLoopBowCand, vpMergeBowCand;
      db.DetectNBestCandidates(current, vpLoopBowCand, vpMergeBowCand, 3);
      db.add(4, 0, a);
      db.erase(2);
      db.clearMap(1);
      std::printf("%zu relocalisation, %zu loop, %zu merge candidates, %zu key frames\n", vpCandidateKFs.size(), vpLoopBowCand.size(),
                  vpMergeBowCand.size(), db.size());
      return vpCandidateKFs.size() == 1 && vpCandidateKFs[0] == 1 && vpLoopBowCand.size() == 1 && vpMergeBowCand.size() == 1 && db.size() == 2 ? 0 : 1;
    }
    Reader r;
    {
      std::ifstream f(argv[2], std::ios::binary);
      r.b.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    }
    const std::vector<int32_t> h = r.take<int32_t>(7);
    size_t maxWords = 1;
    struct Kf { int id, map; DBoW2::BowVector bow; std::vector<int> cov; };
    std::vector<Kf> kfs;
    for (int i = 0; i < h[0]; i++) {
      const std::vector<int32_t> m = r.take<int32_t>(4);
      const std::vector<uint32_t> w = r.take<uint32_t>(m[2]);
      const std::vector<double> v = r.take<double>(m[2]);
      const std::vector<int32_t> c = r.take<int32_t>(m[3]);
      kfs.push_back(Kf{m[0], m[1], bow(w, v), std::vector<int>(c.begin(), c.end())});
      maxWords = std::max(maxWords, w.size());
    }
    const std::vector<int32_t> conn = r.take<int32_t>(h[4]), bad = r.take<int32_t>(h[5]);
    const std::vector<uint32_t> qw = r.take<uint32_t>(h[6]);
    const std::vector<double> qv = r.take<double>(h[6]);
    const DBoW2::BowVector query = bow(qw, qv);
    ORB_SLAM3::KeyFrameDatabase db(voc, (int)kfs.size() + 1, (int)std::max(maxWords, qw.size()));
    for (const Kf& k : kfs) db.add(k.id, k.map, k.bow);
    for (const Kf& k : kfs) db.SetBestCovisibilityKeyFrames(k.id, k.cov);
    std::ofstream o(argv[3], std::ios::binary);
    if (h[1] == 0) {
      write_list(o, db.DetectRelocalizationCandidates(query, h[2]));
    } else {
      ORB_SLAM3::KeyFrameQuery current;
      current.mBowVec = &query;
      current.mnMapId = h[2];
      current.spConnectedKeyFrames.insert(conn.begin(), conn.end());
      std::vector<int> vpLoopBowCand, vpMergeBowCand;
      db.DetectNBestCandidates(current, vpLoopBowCand, vpMergeBowCand, h[3], std::set<int>(bad.begin(), bad.end()));
      db.add(1 << 20, h[2], query);   // mpKeyFrameDB->add(mpCurrentKF)
      write_list(o, vpLoopBowCand);
      write_list(o, vpMergeBowCand);
    }
    return 0;
  } catch (const std::exception& e) {
    std::printf("no-device error: %s\n", e.what());
    return 3;
  }
}
