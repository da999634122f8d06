// orbx_pose_inertial.h — the per-frame argument record of k_pose_inertial (orbx_pose_inertial.hip) and its launcher, shared with
// the C ABI (orbx_api_pose_inertial.hip).  Workgroup size, edge cap and the LDS staging cap are orbx_pose.h's.
#ifndef ORBX_POSE_INERTIAL_H
#define ORBX_POSE_INERTIAL_H
#include "orbx_pose.h"

struct PoseInertialArgs {
  const orbx_keypoint* kps;                  // mvKeysUn, by key point
  const float* uR;                           // mvuRight by key point, nullptr = every edge mono
  const float* wpos;                         // [nE][3] world positions, by edge
  const float* depth;                        // [nE] MapPoint::mTrackDepth, by edge
  const int* eidx;                           // edge -> key point (ascending)
  const orbx_pose_inertial_frame* frame;
  const orbx_imu_state* set1;                // the last key frame (fixed) or the previous frame (free)
  const orbx_imu_prior* prior;               // last frame only
  const orbx_imu_preintegrated* preInertial; // the inertial edge's record
  const orbx_imu_preintegrated* preWalk;     // the record whose C gives the walk edges' information
  float4* stage;                             // 2 * nE float4 when nE > kLdsEdges
  orbx_pose_inertial_result* result;
  uint8_t* eout;                             // outlier flag by edge
  int nE, recInit;
};

// k_pose_inertial<lastFrame> over nFrames records; lds = dynamic LDS bytes for the staged edges
hipError_t launch_pose_inertial(const PoseInertialArgs* d_frames, int nFrames, bool lastFrame, size_t lds, const float* d_invSigma2,
                                int nlevels);
#endif
