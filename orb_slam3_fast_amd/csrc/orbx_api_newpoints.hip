// orbx_api_newpoints.hip — C ABI of the new-map-point geometry (include/orbx.h, "new map points"): orbx_triangulate_matches (one
// pair of key frames, a caller-supplied match list) and orbx_create_new_map_points (the neighbour loop of
// LocalMapping::CreateNewMapPoints: the triangulation search and k_new_points per neighbour on one stream, sharing one
// device-resident has_map_point1).  One Pack per call: one upload, the launches, one download.
#include "orbx_host.h"

namespace {

const char* np_camera_error(const orbx_np_camera& c) {
  if (const char* e = camera_error(c.model, c.p, c.kb8_precision)) return e;
  if (!finite_all(c.Tcw, 12) || !finite_all(c.Ow, 3)) return "key frame pose not finite";
  return nullptr;
}

// everything the kernel trusts about a key frame, checked on the host
const char* np_keyframe_error(const orbx_np_keyframe* f) {
  if (!f) return "null key frame";
  if (f->n < 0 || f->nlevels < 1 || !f->scale_factors || !f->level_sigma2 || (f->n && !f->kps)) return "bad argument";
  if (f->n_cameras != 1 && f->n_cameras != 2) return "n_cameras is neither 1 nor 2";
  if (f->n_cameras == 1 && f->n_left != -1) return "n_left must be -1 for a single-camera key frame";
  if (f->n_cameras == 2 && (f->n_left < 0 || f->n_left > f->n)) return "n_left outside [0, n]";
  if ((f->u_right != nullptr) != (f->depth != nullptr)) return "u_right and depth must both be given or both be NULL";
  if (!std::isfinite(f->mb)) return "mb not finite";
  for (int c = 0; c < f->n_cameras; c++)
    if (const char* e = np_camera_error(f->cam[c])) return e;
  for (int i = 0; i < f->n; i++)
    if (f->kps[i].octave < 0 || f->kps[i].octave >= f->nlevels) return "keypoint octave outside [0, nlevels)";
  return nullptr;
}

const char* np_params_error(const orbx_np_params* p) {
  if (!p) return "null params";
  if (!std::isfinite(p->mbf) || !std::isfinite(p->ratio_factor) || (p->far_points && !std::isfinite(p->th_far)))
    return "params not finite";
  return nullptr;
}

// a key frame's arrays in the call's upload.  withKps false: the keypoints are already there (a BoW side's).
struct KfAreas { size_t kps, raw, ur, depth, scale, sigma; };
KfAreas add_keyframe(Pack& pk, const orbx_np_keyframe& f, bool withKps) {
  KfAreas o{};
  const size_t n = (size_t)f.n;
  if (withKps) o.kps = pk.add(f.kps, n * sizeof(orbx_keypoint));
  const bool stereo = f.n_cameras == 1 && f.u_right;
  if (stereo && f.kps_raw && f.kps_raw != f.kps) o.raw = pk.add(f.kps_raw, n * sizeof(orbx_keypoint));
  if (stereo) {
    o.ur = pk.add(f.u_right, n * 4);
    o.depth = pk.add(f.depth, n * 4);
  }
  o.scale = pk.add(f.scale_factors, (size_t)f.nlevels * 4);
  o.sigma = pk.add(f.level_sigma2, (size_t)f.nlevels * 4);
  return o;
}
NpKf device_keyframe(const Pack& pk, const orbx_np_keyframe& f, const KfAreas& o, const orbx_keypoint* kps) {
  NpKf d{};
  d.cam[0] = f.cam[0];
  d.cam[1] = f.n_cameras == 2 ? f.cam[1] : f.cam[0];
  d.twoCam = f.n_cameras == 2;
  d.nLeft = f.n_left;
  d.n = f.n;
  d.mb = f.mb;
  d.k = kps;
  const bool stereo = f.n_cameras == 1 && f.u_right;
  d.kraw = stereo && f.kps_raw && f.kps_raw != f.kps ? pk.ptr<orbx_keypoint>(o.raw) : kps;
  d.ur = stereo ? pk.ptr<float>(o.ur) : nullptr;
  d.depth = stereo ? pk.ptr<float>(o.depth) : nullptr;
  d.scale = pk.ptr<float>(o.scale);
  d.sigma2 = pk.ptr<float>(o.sigma);
  return d;
}

void fill_np(NewPointsArgs& a, const orbx_np_params& p) {
  a.mbf = p.mbf;
  a.inertial = p.inertial ? 1 : 0;
  a.farPoints = p.far_points ? 1 : 0;
  a.thFar = p.th_far;
  a.ratioFactor = p.ratio_factor;
}

// the output row of one (neighbour, key frame 1) pair inside the download: result | matches | x3d | status | point_stereo
struct RowAreas { size_t res, x3d, status, ps; };
RowAreas add_row(Pack& pk, size_t n, bool withMatches) {
  RowAreas r{};
  if (withMatches) r.res = pk.add(nullptr, (n + 1) * 4);
  r.x3d = pk.add(nullptr, n * 12);
  r.status = pk.add(nullptr, n);
  r.ps = pk.add(nullptr, n);
  return r;
}

int count_created(const uint8_t* status, int n) {
  int c = 0;
  for (int i = 0; i < n; i++) c += status[i] == ORBX_NP_CREATED;
  return c;
}

}  // namespace

extern "C" {

int orbx_triangulate_matches(int device, const orbx_np_keyframe* kf1, const orbx_np_keyframe* kf2, const int32_t* matches12,
                             const orbx_np_params* params, uint8_t* status, float* x3d, uint8_t* point_stereo) {
  const char* err;
  if ((err = np_keyframe_error(kf1)) || (err = np_keyframe_error(kf2)) || (err = np_params_error(params)))
    return fail(ORBX_E_BADARG, err);
  if (kf1->n_cameras != kf2->n_cameras) return fail(ORBX_E_BADARG, "both key frames must be single-camera or both two-camera");
  const int n1 = kf1->n, n2 = kf2->n;
  if (n1 && (!matches12 || !status || !x3d || !point_stereo)) return fail(ORBX_E_BADARG, "bad argument");
  for (int i = 0; i < n1; i++)
    if (matches12[i] < -1 || matches12[i] >= n2) return fail(ORBX_E_BADARG, "match index outside [-1, n2)");
  int rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  if (n1 == 0) return 0;
  Pack pk;
  const KfAreas o1 = add_keyframe(pk, *kf1, true), o2 = add_keyframe(pk, *kf2, true);
  const size_t oM = pk.add(matches12, (size_t)n1 * 4);
  const RowAreas row = add_row(pk, (size_t)n1, false);
  hipError_t e = pk.commit();
  NewPointsArgs a{};
  a.kf1 = device_keyframe(pk, *kf1, o1, pk.ptr<orbx_keypoint>(o1.kps));
  a.kf2 = device_keyframe(pk, *kf2, o2, pk.ptr<orbx_keypoint>(o2.kps));
  a.match = pk.ptr<int>(oM);
  fill_np(a, *params);
  a.x3d = pk.ptr<float>(row.x3d); a.status = pk.ptr<uint8_t>(row.status); a.pointStereo = pk.ptr<uint8_t>(row.ps);
  if (e == hipSuccess) e = launch_new_points(a, nullptr);
  if (e == hipSuccess) {
    const uint8_t* h = pk.fetch(row.x3d, row.ps + (size_t)n1 - row.x3d, &e);
    if (e == hipSuccess) {
      std::memcpy(x3d, h, (size_t)n1 * 12);
      std::memcpy(status, h + (row.status - row.x3d), (size_t)n1);
      std::memcpy(point_stereo, h + (row.ps - row.x3d), (size_t)n1);
    }
  }
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  return count_created(status, n1);
}

int orbx_create_new_map_points(int device, const orbx_np_keyframe* kf1, const orbx_np_bow* bow1, const orbx_np_neighbour* neighbours,
                               int n_neighbours, const orbx_np_params* params, int32_t* n_matches, int32_t* n_created,
                               int32_t* matches12, uint8_t* status, float* x3d, uint8_t* point_stereo, uint8_t* has_map_point1_out) {
  const int K = n_neighbours;
  const char* err;
  if ((err = np_keyframe_error(kf1)) || (err = np_params_error(params))) return fail(ORBX_E_BADARG, err);
  if (K < 0 || K > ORBX_NP_MAX_NEIGHBOURS) return fail(ORBX_E_BADARG, "n_neighbours outside [0, 30]");
  if (kf1->n_cameras != 1) return fail(ORBX_E_BADARG, "the chained entry takes single-camera key frames");
  const int n1 = kf1->n;
  if (!bow1 || bow1->n_nodes < 0 || (K && (!neighbours || !n_matches || !n_created)) ||
      (n1 && (!bow1->desc || !bow1->has_map_point || !has_map_point1_out)) ||
      (n1 && K && (!matches12 || !status || !x3d || !point_stereo)) ||
      (bow1->n_nodes && (!bow1->node_ids || !bow1->node_start || !bow1->feature_idx)))
    return fail(ORBX_E_BADARG, "bad argument");
  const BowSide s1{bow1->node_ids, bow1->node_start, bow1->feature_idx, bow1->n_nodes, kf1->kps, bow1->desc, bow1->has_map_point, n1};
  if (s1.list() < 0 || s1.list() > n1) return fail(ORBX_E_BADARG, "feature vector larger than the key frame");
  int rc;
  if ((rc = check_nodes(s1, "feature vector 1")) || (rc = check_features(s1, "feature index 1"))) return rc;
  std::vector<BowSide> s2(K);
  std::vector<char> skip(K, 0);
  for (int k = 0; k < K; k++) {
    const orbx_np_neighbour& nb = neighbours[k];
    if ((err = np_keyframe_error(&nb.kf))) return fail(ORBX_E_BADARG, err);
    if (nb.kf.n_cameras != 1) return fail(ORBX_E_BADARG, "the chained entry takes single-camera key frames");
    const orbx_np_bow& b = nb.bow;
    if (b.n_nodes < 0 || (nb.kf.n && (!b.desc || !b.has_map_point)) || (b.n_nodes && (!b.node_ids || !b.node_start || !b.feature_idx)))
      return fail(ORBX_E_BADARG, "bad argument");
    s2[k] = BowSide{b.node_ids, b.node_start, b.feature_idx, b.n_nodes, nb.kf.kps, b.desc, b.has_map_point, nb.kf.n};
    if (s2[k].list() < 0 || s2[k].list() > nb.kf.n) return fail(ORBX_E_BADARG, "feature vector larger than the key frame");
    if (s2[k].list() >= (1 << 24)) return fail(ORBX_E_CAPACITY, "more than 2^24 features");
    if ((rc = check_nodes(s2[k], "feature vector 2")) || (rc = check_features(s2[k], "feature index 2"))) return rc;
    if (!finite_all(nb.ep, 2) || (!params->coarse && !finite_all(nb.F12, 9))) return fail(ORBX_E_BADARG, "epipole or F12 not finite");
    // the baseline test (:466-478) in the reference's float arithmetic
    const float bx = nb.kf.cam[0].Ow[0] - kf1->cam[0].Ow[0], by = nb.kf.cam[0].Ow[1] - kf1->cam[0].Ow[1],
                bz = nb.kf.cam[0].Ow[2] - kf1->cam[0].Ow[2];
    const float baseline = std::sqrt(bx * bx + by * by + bz * bz);
    if (!params->monocular) {
      skip[k] = baseline < nb.kf.mb;
    } else {
      if (!std::isfinite(nb.median_depth)) return fail(ORBX_E_BADARG, "median_depth not finite");
      const float ratioBaselineDepth = baseline / nb.median_depth;
      skip[k] = (double)ratioBaselineDepth < 0.01;
    }
  }
  rc = set_device(device);
  if (rc != ORBX_OK) return rc;
  const size_t N1 = (size_t)n1;
  int total = 0;
  for (int k = 0; k < K; k++) {   // the rows of a skipped neighbour; the others are overwritten by the download
    n_matches[k] = skip[k] ? -1 : 0;
    n_created[k] = 0;
    for (size_t i = 0; i < N1; i++) matches12[k * N1 + i] = -1;
    if (n1) {
      std::memset(status + k * N1, ORBX_NP_NO_MATCH, N1);
      std::memset(point_stereo + k * N1, 0, N1);
      std::memset(x3d + k * N1 * 3, 0, N1 * 12);
    }
  }
  if (n1) std::memcpy(has_map_point1_out, bow1->has_map_point, N1);
  if (n1 == 0 || K == 0) return 0;

  Pack pk;
  const SideAreas b1 = add_side(pk, s1);
  const KfAreas o1 = add_keyframe(pk, *kf1, false);
  std::vector<SideAreas> b2(K);
  std::vector<KfAreas> o2(K);
  for (int k = 0; k < K; k++) {
    if (skip[k]) continue;
    b2[k] = add_side(pk, s2[k]);
    o2[k] = add_keyframe(pk, neighbours[k].kf, false);
  }
  std::vector<size_t> oFlags(K);
  for (int k = 0; k < K; k++)
    if (!skip[k]) oFlags[k] = pk.add(nullptr, 33 * 4);
  // outputs: the working copy of has_map_point1, then one row per neighbour -- one copy back
  const size_t oMp = pk.add(nullptr, N1);
  std::vector<RowAreas> row(K);
  size_t outEnd = oMp + N1;
  for (int k = 0; k < K; k++) {
    if (skip[k]) continue;
    row[k] = add_row(pk, N1, true);
    outEnd = row[k].ps + N1;
  }
  hipError_t e = pk.commit();
  uint8_t* mp1 = pk.ptr<uint8_t>(oMp);
  if (e == hipSuccess) e = hipMemcpyAsync(mp1, pk.ptr<uint8_t>(b1.flags), N1, hipMemcpyDeviceToDevice, nullptr);
  for (int k = 0; k < K && e == hipSuccess; k++) {
    if (skip[k]) continue;
    const orbx_np_neighbour& nb = neighbours[k];
    TriArgs t = tri_args(pk, s1, b1, s2[k], b2[k]);
    t.mp1 = mp1;
    NewPointsArgs a{};
    a.kf1 = device_keyframe(pk, *kf1, o1, t.k1);
    a.kf2 = device_keyframe(pk, nb.kf, o2[k], t.k2);
    t.ur1 = a.kf1.ur; t.ur2 = a.kf2.ur;
    t.scale2 = a.kf2.scale; t.sigma2 = a.kf2.sigma2;
    t.ep0 = nb.ep[0]; t.ep1 = nb.ep[1];
    for (int i = 0; i < 9; i++) t.F[i] = params->coarse ? 0.f : nb.F12[i];
    t.onlyStereo = params->only_stereo ? 1 : 0; t.coarse = params->coarse ? 1 : 0; t.checkOri = params->check_orientation ? 1 : 0;
    t.flags = pk.ptr<int>(oFlags[k]); t.result = pk.ptr<int>(row[k].res); t.match = t.result + 1;
    e = launch_search_for_triangulation(t, nullptr);
    if (e != hipSuccess) break;
    a.match = t.match;
    fill_np(a, *params);
    a.x3d = pk.ptr<float>(row[k].x3d); a.status = pk.ptr<uint8_t>(row[k].status); a.pointStereo = pk.ptr<uint8_t>(row[k].ps);
    a.mp1 = mp1;
    e = launch_new_points(a, nullptr);
  }
  if (e == hipSuccess) {
    const uint8_t* h = pk.fetch(oMp, outEnd - oMp, &e);
    if (e == hipSuccess) {
      std::memcpy(has_map_point1_out, h, N1);
      for (int k = 0; k < K; k++) {
        if (skip[k]) continue;
        const RowAreas& r = row[k];
        std::memcpy(&n_matches[k], h + (r.res - oMp), 4);
        std::memcpy(matches12 + k * N1, h + (r.res - oMp) + 4, N1 * 4);
        std::memcpy(x3d + k * N1 * 3, h + (r.x3d - oMp), N1 * 12);
        std::memcpy(status + k * N1, h + (r.status - oMp), N1);
        std::memcpy(point_stereo + k * N1, h + (r.ps - oMp), N1);
        n_created[k] = count_created(status + k * N1, n1);
        total += n_created[k];
      }
    }
  }
  if (e != hipSuccess) return fail(ORBX_E_HIP, hipGetErrorString(e));
  return total;
}

}  // extern "C"
