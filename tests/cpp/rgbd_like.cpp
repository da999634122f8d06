// Drives ORBextractor::ExtractRGBD the way the reference's RGB-D Frame constructor would call it (src/Frame.cc:281-348, with
// Tracking::GrabImageRGBD's depth conversion folded in): one gray image, its RAW depth image, mDepthMapFactor, K, mDistCoef and
// mbf in; mvKeys, mDescriptors, mvKeysUn, mvuRight and mvDepth out as flat binary files for tests/test_rgbd_cpp.py.
//   usage: rgbd_like <w> <h> <nfeat> <gray.raw> <depth.raw> <depth_type 2|5> <depth_scale> <bf> <fx> <fy> <cx> <cy>
//                    <n_dist> <d0 ...> <outprefix>
// Without arguments it only constructs the extractor: exit 3 and "no-device error" without a GPU.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../orb_slam3_fast_amd/csrc/ORBextractor.h"

using namespace ORB_SLAM3;

static std::vector<uint8_t> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
template <class T>
static void dump(const std::string& path, const T* p, size_t n) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T)));
}

int main(int argc, char** argv) {
  if (argc < 2) {
    try {
      ORBextractor ex(1000, 1.2f, 8, 20, 7, 640, 480);
      std::printf("constructed on a GPU\n");
      return 0;
    } catch (const std::exception& e) {
      std::printf("no-device error: %s\n", e.what());
      return 3;
    }
  }
  if (argc < 15) {
    std::printf("usage: rgbd_like w h nfeat gray.raw depth.raw type scale bf fx fy cx cy n_dist d... outprefix\n");
    return 2;
  }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), nf = std::atoi(argv[3]);
  std::vector<uint8_t> gray = slurp(argv[4]), dep = slurp(argv[5]);
  const int type = std::atoi(argv[6]);
  const float scale = std::strtof(argv[7], nullptr), bf = std::strtof(argv[8], nullptr);
  const float K[4] = {std::strtof(argv[9], nullptr), std::strtof(argv[10], nullptr), std::strtof(argv[11], nullptr),
                      std::strtof(argv[12], nullptr)};
  const int nd = std::atoi(argv[13]);
  if (argc != 15 + nd) {
    std::printf("expected %d distortion coefficients\n", nd);
    return 2;
  }
  std::vector<float> dist;
  for (int i = 0; i < nd; i++) dist.push_back(std::strtof(argv[14 + i], nullptr));
  const std::string out = argv[14 + nd];
  const size_t es = type == 2 ? 2 : 4;
  if (gray.size() != (size_t)w * h || dep.size() != (size_t)w * h * es) {
    std::printf("input sizes do not match %dx%d\n", w, h);
    return 2;
  }
  try {
    ORBextractor ex(nf, 1.2f, 8, 20, 7, w, h);
#ifdef ORBX_HAVE_OPENCV
    cv::Mat imGray(h, w, CV_8UC1, gray.data(), (size_t)w);
    cv::Mat imDepth(h, w, type, dep.data(), (size_t)w * es);
#else
    ocv::Mat imGray(h, w, gray.data(), (size_t)w);
    ocv::Mat imDepth(h, w, type, dep.data(), (size_t)w * es);
#endif
    std::vector<ocv::KeyPoint> keys, keysUn;
    ocv::Mat desc;
    std::vector<float> uRight, depth;
    // twice, as consecutive frames of a sequence: the second call must not see anything of the first
    ex.ExtractRGBD(imGray, imDepth, scale, K, dist, bf, keys, desc, keysUn, uRight, depth);
    const int mono = ex.ExtractRGBD(imGray, imDepth, scale, K, dist, bf, keys, desc, keysUn, uRight, depth);
    const size_t n = keys.size();
    dump(out + ".k", keys.data(), n);
    dump(out + ".d", desc.data, n * 32);
    dump(out + ".kun", keysUn.data(), keysUn.size());
    dump(out + ".ur", uRight.data(), uRight.size());
    dump(out + ".dep", depth.data(), depth.size());
    std::printf("%d %zu\n", mono, n);
  } catch (const std::exception& e) {
    std::printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
