// orbx_lba.h — what the local bundle adjustment's kernels (orbx_lba.hip) and its C ABI (orbx_api_lba.hip) share: the argument
// record of the kernel chain, the device-resident Levenberg state and the launches.
#ifndef ORBX_LBA_H
#define ORBX_LBA_H
#include "orbx_host.h"
#include "orbx_optim.h"

#include <vector>

namespace orbx {

constexpr int kLbaApp = 27;   // per edge: the key frame's 6 x 6 block (upper triangle, 21) and its share of b (6)
constexpr int kLbaAll = 9;    // per edge: the point's 3 x 3 block (upper triangle, 6) and its share of b (3)
constexpr int kLbaHpl = 18;   // per edge: the 6 x 3 pose-point block, row-major

struct LbaPose { double q[4], t[3]; };
struct LbaRigTrl { LbaPose T; double R[3][3]; };   // SE3Quat(Trl) normalised, and its toRotationMatrix

// The optimiser's state (optimization_algorithm_levenberg.cpp), written by k_lba_decide's thread 0 only.  `cur` names the copy
// of the estimates and of the linear system (0 / 1) that belongs to the current estimate; a trial is built in the other copy.
struct LbaState {
  LmState lm;          // the Levenberg rule's own fields (orbx_optim.h)
  double chiInitial;
  int cur, stage, trials, ok, running, stopReason;
};

// What the step between the two optimisations of the map-merge bundle adjustment writes (k_lba_relevel, k_lba_relayout): round
// two reads these through LbaArgs::level / ptLive / slot / row.
struct LbaRelevel {
  uint8_t* level;     // [nE] 1: the edge was put aside after round one (setLevel(1))
  int* ptLive;        // [nP] level-0 edges of the point
  int* slot;          // [nKF] row block of round two's reduced system, -1: not in its active set
  int* row;           // [nOpt] round two's slot -> round one's slot, the row of kfStart
  int* counts;        // round two's nOpt, the number of level-1 edges
  double* scalars;    // round one's lambda, chi2_initial, chi2_final
  int* counters;      // round one's iterations, trials, stop_reason
};

struct LbaArgs {
  const orbx_lba_keyframe* kfs;   // [nKF]
  const orbx_lba_edge* edges;     // [nE]
  const float* points;            // [nP][3]
  const int* slot;                // [nKF] row block of the reduced system, -1: not optimised
  const int* ptStart;             // [nP + 1] a point's edges are [ptStart[p], ptStart[p + 1])
  const int* kfStart;             // [nOpt + 1] CSR of a slot's edges, ascending
  const int* kfEdges;
  LbaPose* pose[2];               // [nKF] estimates, two copies
  double* X[2];                   // [nP][3]
  double* hpl[2];                 // [nE][kLbaHpl]
  double* hpp[2];                 // [nOpt][kLbaApp]: Hpp (21), bp (6)
  double* hll[2];                 // [nP][kLbaAll]: Hll (6), bl (3)
  double* eApp;                   // [nE][kLbaApp] the edges' terms of the pass, reduced right away
  double* eAll;                   // [nE][kLbaAll]
  double* eRho;                   // [nE] robust chi2 of the pass
  double* ptChi;                  // [nP] its per-point sums
  double* dinv;                   // [nP][6] (Hll + lambda I)^-1, upper triangle
  double* S;                      // [n][n] the reduced camera system, row-major; the factorisation's workspace (lower triangle)
  double* bs;                     // [n]
  double* xp;                     // [n] pose increments
  double* xl;                     // [nP][3] point increments
  LbaState* st;
  // outputs, one contiguous area
  int* status;                    // running flag of the last decision (the host's one word per trial)
  double* outPose;                // [nLocal][7]
  double* outPts;                 // [nP][3]
  double* chi2;                   // [nE] the chi2 every edge holds (written by every linearisation)
  uint8_t* erase;                 // [nE]
  uint8_t* depthPos;              // [nE]
  double* outScalars;             // lambda, chi2_initial, chi2_final
  int* outCounters;               // iterations, trials, stop_reason
  int nKF, nLocal, nP, nE, nOpt, n, maxIter;
  double lambdaInit;
  // what the local and the full bundle adjustment differ by
  int robust;                     // 0: no robust kernel (rho' = 1, the chi2 is the plain sum)
  int blocked;                    // the linear solve: 0 k_lba_solve (n <= 6 ORBX_LBA_MAX_LOCAL), 1 the blocked LDLT of orbx_ba.hip
  double deltaMono, deltaStereo;  // Huber deltas, already narrowed to float and widened as the reference holds them
  // The rig entries only.  cams == nullptr is the pinhole chain, which reads none of these, and the launches choose the kernels
  // by it: every site that fills an LbaArgs or an LbaConfig value-initialises it (`LbaArgs a{}`, `LbaConfig cfg{}`), and the old
  // entries leave these fields alone.  A record built any other way must set cams = nullptr itself.
  const orbx_lba_rig_camera* cams;   // [nKF]
  const uint8_t* edgeCam;            // [nE] 0 left, 1 second camera
  LbaRigTrl* trl;                    // [nKF] mTrl as the edges hold it, written by k_lba_rig_init
  // The map-merge entries only (orbx_api_merge_ba.hip).  level == nullptr is every other call: no edge is masked, a slot is its
  // own row of kfStart and the points' and key frames' active sets are what ptStart and slot say.  Round two of the merge entries
  // sets all four to LbaRelevel's arrays and slot to LbaRelevel::slot: the kernels skip level-1 edges and what has no level-0 edge.
  const uint8_t* level;              // [nE]
  const int* ptLive;                 // [nP]
  const int* row;                    // [nOpt]
  const int* slot0;                  // [nKF] round one's slot: the key frames whose estimate comes back (nullptr: slot)
  LbaRelevel rl;
};

// ---- the host side the two bundle adjustments' entries share (orbx_api_lba.hip)
constexpr int kLbaMaxIterations = 1000000;

// what the validation derives from a problem
struct LbaLayout {
  std::vector<int> ptStart;   // [nP + 1]
  std::vector<int> slot;      // [nKF] row block of the reduced system, -1: not optimised
  std::vector<int> deg;       // [nKF] edges of the key frame
  int nOpt = 0, fixedLocal = 0;
};

struct LbaConfig {
  int maxIterations;
  float lambdaInit;
  int robust, blocked;
  float deltaMono, deltaStereo;        // narrowed, as the reference's thHuber* are floats
  const volatile int32_t* stopFlag;    // nullptr: never asked
  int nPoses;                          // the first nPoses key frames come back
  const orbx_lba_rig_camera* cams;     // the rig entries: the kernels of the rig chain; nullptr: the pinhole chain
  const uint8_t* edgeCam;
  // the map-merge entries: secondIterations > 0 runs a second optimize() over the edges that pass the classification, without
  // robust kernels, unless the stop flag was seen by then
  int secondIterations;
  int stopAfterFirst;                  // tests: the stop flag counts as seen right behind round one
};

// outputs of a run; chi2 / erase / depthPos may be nullptr
struct LbaRun {
  double* poses;
  double* points;
  double* chi2;
  uint8_t* erase;
  uint8_t* depthPos;
  int stopped, iterations, trials, stopReason;   // of the last optimize() that ran
  double lambda, chiInitial, chiFinal;
  // the map-merge entries (LbaConfig::secondIterations > 0)
  uint8_t* level;                                // [nE], may be nullptr
  int rounds, nLevel1;                           // optimize() calls that were reached; edges put aside
  int firstIterations, firstTrials, firstStopReason;   // round one, when rounds == 2
  double firstLambda, firstChiInitial, firstChiFinal;
};

// every check of a problem that needs no device, in the order the entries report them; fills g
// cams != nullptr: the checks of the rig entries (KB8 key frames, second cameras, one edge per camera and pair)
const char* lba_graph_error(const orbx_lba_problem& p, int maxIterations, float lambdaInit, LbaLayout& g,
                            const orbx_lba_rig_camera* cams = nullptr, const uint8_t* edgeCam = nullptr);
void lba_passthrough(const orbx_lba_problem& p, int nPoses, LbaRun& r);   // the widened inputs, every counter zero
// upload, the chain of trials (the stop flag asked in front of the first and after each), download
int lba_optimise(int device, const orbx_lba_problem& p, const LbaLayout& g, const LbaConfig& cfg, LbaRun& r);

// the chain on the null stream (orbx_lba.hip)
// a.cams != nullptr: k_lba_linearize_rig, k_lba_schur_rig and k_lba_finish_rig take the places of the pinhole kernels
hipError_t launch_lba_init(const LbaArgs& a);       // estimates from the inputs, the state, x = 0 (rig: and every mTrl)
hipError_t launch_lba_evaluate(const LbaArgs& a);   // linearise at the estimate (stage 0) or the trial, reduce, decide
hipError_t launch_lba_trial(const LbaArgs& a);      // Dinv, Schur complement, factorisation and solve, back-substitution, oplus
hipError_t launch_lba_finish(const LbaArgs& a);     // classification and outputs
// between the rounds of the map-merge entries: the levels by k_lba_finish's erase rule, round two's layout into a.rl, a fresh state
hipError_t launch_lba_relevel(const LbaArgs& a);
// k_lba_solve alone, as launch_lba_trial launches it: reads n, S, bs; writes xp (when every pivot holds) and st->ok
hipError_t launch_lba_solve(const LbaArgs& a);

}  // namespace orbx
#endif
