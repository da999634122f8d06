/* orbx.h — C ABI of the MI355X-native ORB front-end (liborbx.so).
 *
 * Drop-in boundary for the reference's ORB hot path (hellovuong/ORB_SLAM3_FAST).  Every entry point names
 * the reference interface it replaces (file:line relative to the reference root).  Plain pointers and
 * sizes only: no OpenCV, no torch types.  The C++ mirror classes ORB_SLAM3::ORBextractor / ORBmatcher in
 * orb_slam3_fast_amd/csrc/ORBextractor.h / ORBmatcher.h sit on top of exactly these calls; INTEGRATION.md
 * shows the binding a maintainer of the reference would add.
 *
 * All compute runs in hand-written HIP kernels for gfx950.  There is no CPU fallback: without a HIP device
 * every compute call returns ORBX_E_NODEVICE / ORBX_E_HIP.
 */
#ifndef ORBX_H_
#define ORBX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_MAX_LEVELS 12

/* Error codes.  ORBX_E_EMPTY keeps ORBextractor::operator()'s "-1 on empty image"
 * (src/ORBextractor.cc:1021). */
#define ORBX_OK 0
#define ORBX_E_EMPTY (-1)
#define ORBX_E_BADARG (-2)
#define ORBX_E_CAPACITY (-3)
#define ORBX_E_HIP (-4)
#define ORBX_E_NODEVICE (-5)
#define ORBX_E_UNSUPPORTED (-6) /* image too small for the pyramid or aspect (Q11) */
#define ORBX_E_TIMEOUT (-7)     /* orbx_comm_wait: a collective did not complete in time (a rank missing / out of order) */

/* Layout-identical to cv::KeyPoint (28 bytes): pt.x pt.y size angle response octave class_id
 * (SURVEY 8a row a13). */
typedef struct orbx_keypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} orbx_keypoint;

/* Constructor arguments of ORBextractor (include/ORBextractor.h:53-57, src/ORBextractor.cc:408-417). */
typedef struct orbx_params {
  int32_t nfeatures;
  float scale_factor;
  int32_t nlevels;
  int32_t ini_th_fast;
  int32_t min_th_fast;
} orbx_params;

typedef struct orbx_extractor orbx_extractor;

const char* orbx_last_error(void);
int orbx_device_count(void);
int orbx_abi_version(void);

/* ---- ORBextractor ---------------------------------------------------------------------------------- */

/* Replaces ORBextractor::ORBextractor (src/ORBextractor.cc:408-469).  One handle = one extractor instance
 * bound to `device` with its own HIP stream; it owns pyramids and result buffers for up to max_batch images
 * of up to max_width x max_height per call.  Handles are not re-entrant (like the reference instance, which
 * mutates mvImagePyramid); distinct handles may be used concurrently from different threads
 * (src/Frame.cc:200-203). */
int orbx_extractor_create(const orbx_params* p, int max_width, int max_height, int max_batch, int device,
                          orbx_extractor** out);
void orbx_extractor_destroy(orbx_extractor* ex);

/* Replaces GetScaleFactors/GetInverseScaleFactors/GetScaleSigmaSquares/GetInverseScaleSigmaSquares
 * (include/ORBextractor.h:65-83) plus the private mnFeaturesPerLevel / umax tables.  Any pointer may be
 * NULL.  Arrays hold nlevels entries, umax16 holds 16. */
int orbx_get_tables(const orbx_extractor* ex, float* scale, float* inv_scale, float* sigma2,
                    float* inv_sigma2, int32_t* nfeatures_per_level, int32_t* umax16);

/* Which OpenCV the reference build links decides the descriptor bits: cv::GaussianBlur(7x7, sigma 2) of ORBextractor::operator()
 * (src/ORBextractor.cc:1074-1076) runs on 8-bit fixed-point taps that changed between releases -- {18,34,49,55,49,34,18} / 256 in
 * OpenCV 4.0 .. 4.5.0 (the README's "tested with 4.4.0", README.md:101; the taps sum to 257, results saturate at 255) and
 * {18,34,48,56,48,34,18} / 256 from 4.5.1 on (CMakeLists.txt:38-41 asks for "> 4.4"; what distributions ship).
 * opencv_version = 451 (the default), 440, 44016 or 44032; anything else is ORBX_E_BADARG.  Applies to every later extraction of
 * the handle (k_describe's per-keypoint blur and the blurred levels of orbx_pyramid_level).  OpenCV 3.x's float filter is not
 * modelled.
 *   440   : the 257-sum taps through the SCALAR ufixedpoint path, every column rounded once.
 *   44016 / 44032 : the same taps as a build whose vertical pass runs the 16-lane (SSE2 / NEON baseline) or 32-lane (AVX2
 *           dispatch) vector body of smooth.simd.hpp: that body re-biases its 8.8 rows by -32768 and gives the bias back as the
 *           constant 128 << 16, which is 32768 short when the taps sum to 257 -- exactly the rounding half, so columns
 *           [0, (w / lanes) * lanes) of every level FLOOR and only the scalar tail behind them rounds (flat 100 -> 100 in the
 *           body, 101 in the tail; oracle/orb_oracle.cpp gaussian_blur7, tests/test_tables.py).  A reference built against
 *           OpenCV 4.4.0 on x86-64 is expected to behave as 44032.
 * STATUS: all settings follow this repo's restatement of OpenCV's fixed-point path (oracle/orb_oracle.cpp gaussian_blur7), which
 * is not pinned against any real OpenCV build (none exists in this environment); tools/gen_golden_opencv.py with opencv-python
 * 4.4.0 would settle which of 440 / 44016 / 44032 a given build is -- switching is this one call. */
int orbx_set_opencv_compat(orbx_extractor* ex, int opencv_version);

/* Replaces ORBextractor::operator() (src/ORBextractor.cc:1015-1106) for ONE host image (CV_8UC1, `stride`
 * bytes per row).  lap0/lap1 = vLappingArea.  Writes *n_out keypoints (serial-order slots: mono from the
 * front, lapping from the back) and n_out x 32 descriptor bytes.  Returns monoIndex (>= 0), ORBX_E_EMPTY for
 * an empty image, or another negative error.  cap = capacity of kps / desc rows: the handle's own row count
 * (orbx_batch_results_device's *capacity = nfeatures + 36 per level) always suffices; the reference returns at most
 * nfeatures + 3 per level for the usual quotas, but a level whose quota is below 4 x its initial quadtree roots can keep up
 * to 4 * nIni nodes (src/ORBextractor.cc:575-601), so nfeatures + 3 * nlevels is NOT a bound for tiny nfeatures.  ORBX_E_CAPACITY
 * when the result does not fit.  kps / desc may be NULL: the results stay in the handle's result block (orbx_host_results). */
int orbx_extract(orbx_extractor* ex, const uint8_t* img, int w, int h, ptrdiff_t stride, int lap0, int lap1,
                 orbx_keypoint* kps, uint8_t* desc, int cap, int* n_out);

/* Both eyes of ONE stereo frame through one batched pipeline and one synchronisation: replaces the two threaded
 * ExtractORB calls of the stereo Frame constructor (src/Frame.cc:200-203, 549-560) and, when bf > 0, the
 * ComputeStereoMatches that follows them (:921-1084; b = baseline, maxD = bf / b).  The handle needs max_batch >= 2; the
 * left eye becomes image 0 and the right eye image 1 of the extraction (orbx_pyramid_level, orbx_stereo_match_batch with
 * left == right handle, first_left 0, first_right 1).  Outputs as orbx_extract for each eye (n_* keypoints, mono_* =
 * monoIndex); uright / depth (cap_left floats each, -1 = no match) are ignored when bf <= 0.  COMPATIBILITY (since round 5): bf > 0
 * runs the stereo association also when uright / depth are NULL -- the results then wait in the result block
 * (orbx_host_results) --; pass bf = 0 to skip it.  Any of the output ARRAYS
 * (kps_*, desc_*, uright, depth) may be NULL: the results then stay in the handle's page-locked result block, where
 * orbx_host_results hands them out in place (one copy less per frame for a caller that converts them anyway).  Arrays that ARE
 * passed cost nothing at the end of the call: keypoints and descriptors of both eyes reach the block two launches before the frame
 * ends and are copied into the caller's memory while the stereo association still runs (1280x720, 1500 features: 0.183 - 0.20 ms per
 * call either way, profiles/r5c_latency_ab.txt).
 * Returns ORBX_OK, ORBX_E_EMPTY for an empty image, or another negative error. */
int orbx_extract_stereo(orbx_extractor* ex, const uint8_t* img_left, const uint8_t* img_right, int w, int h,
                        ptrdiff_t stride_left, ptrdiff_t stride_right, const int32_t lap_left[2],
                        const int32_t lap_right[2], orbx_keypoint* kps_left, uint8_t* desc_left, int cap_left,
                        int* n_left, int* mono_left, orbx_keypoint* kps_right, uint8_t* desc_right, int cap_right,
                        int* n_right, int* mono_right, float bf, float b, float* uright, float* depth);

/* Results of the last orbx_extract / orbx_extract_stereo call IN PLACE.  Those entries gather everything into one page-locked
 * block owned by the handle (one kernel, one synchronisation) and then copy into the caller's arrays; this accessor exposes
 * the block itself: n keypoints (28-byte cv::KeyPoint records, src/ORBextractor.cc:1053-1104 order) and n x 32 descriptor
 * bytes of image 0 (left eye) or 1 (right eye), monoIndex, and -- image 0 after a call with bf > 0 -- mvuRight / mvDepth
 * (src/Frame.cc:921-1084), n floats each.  Any output pointer may be NULL.  Valid until the next call on the handle. */
int orbx_host_results(const orbx_extractor* ex, int image, const orbx_keypoint** kps, const uint8_t** desc, int* n, int* mono,
                      const float** uright, const float** depth);

/* Batched many-camera mode: n_images device-resident images (image i at d_images + i*image_pitch, rows
 * row_pitch bytes apart; base and pitches 4-byte aligned), all w x h.  d_lap = n_images x 2 int32 lapping
 * areas on the HOST (NULL = all {0,0} as the rectified stereo callers pass, src/Frame.cc:200-201).
 * Enqueues the whole extraction on the handle's stream and returns without synchronising; the images must
 * stay valid until orbx_sync (level 0 of the pyramid aliases them). */
int orbx_extract_batch_device(orbx_extractor* ex, const uint8_t* d_images, int n_images, int w, int h,
                              ptrdiff_t row_pitch, ptrdiff_t image_pitch, const int32_t* lap);
int orbx_sync(orbx_extractor* ex);
/* The HIP stream (hipStream_t, returned as void*) the handle enqueues on: lets a caller queue its own consumers of the
 * device-resident results (a collective over the descriptor blocks, a copy) behind the extraction without a host
 * synchronisation.  The stream belongs to the handle. */
int orbx_stream_handle(const orbx_extractor* ex, void** stream);
/* The same batch from HOST memory (ideally page-locked: then the upload overlaps other handles' kernels): the frames
 * are uploaded into the handle's staging area with asynchronous copies on its stream, the extraction is enqueued behind
 * them, nothing synchronises.  The host frames must stay valid until orbx_sync. */
int orbx_extract_batch(orbx_extractor* ex, const uint8_t* images, int n_images, int w, int h, ptrdiff_t row_pitch,
                       ptrdiff_t image_pitch, const int32_t* lap);
/* All results of the last batch into HOST arrays with asynchronous copies on the handle's stream (page-locked arrays keep
 * them asynchronous): counts[n] / mono[n], kps[n][cap], desc[n][cap][32] (cap = orbx_batch_results_device's cap) and, when
 * n_pairs > 0 and a stereo association ran on this handle, uright / depth [n_pairs][cap].  NULL pointers are skipped.  The
 * arrays are complete after orbx_sync. */
int orbx_batch_download_async(orbx_extractor* ex, int32_t* counts, int32_t* mono, orbx_keypoint* kps, uint8_t* desc,
                              float* uright, float* depth, int n_pairs);

/* ---- Cross-camera descriptor exchange of the batched many-camera mode (BASELINE config C5).
 * The reference has no counterpart: it drives ONE rig per process (Frame's process-global statics,
 * include/Frame.h:230-235,314-319); north_star adds "RCCL over xGMI only for the optional cross-camera descriptor
 * all-gather", one process per GPU.  orbx_comm wraps an RCCL communicator (ncclComm_t):
 *   rank 0: orbx_comm_unique_id(id); the caller ships the 128 bytes to the other ranks (MPI, a file, torch.distributed);
 *   every rank: orbx_comm_create(id, n_ranks, rank, device, &comm)            (collective: all ranks must call it)
 *   or, for a process that already owns an ncclComm_t: orbx_comm_adopt(comm, device, &c) (not destroyed by liborbx).
 * orbx_allgather_descriptors enqueues, on the handle's own stream (behind the extraction, no host synchronisation),
 * ONE grouped RCCL call that gathers the first n_images images' results of the last batch from every rank, straight
 * from the handle's result arrays (no pack step, no staging copy):
 *   d_all_desc   [n_ranks][n_images][cap][32] u8    (cap = orbx_batch_results_device's cap; rows >= count are stale)
 *   d_all_counts [n_ranks][n_images] int32
 * ordered by rank, then by the rank's local image index.  Both destinations are DEVICE arrays owned by the caller and are
 * complete after orbx_sync (or for any work queued later on orbx_stream_handle's stream).  Every rank must call it with the
 * same n_images and a handle of the same capacity.  Errors: ORBX_E_UNSUPPORTED when no RCCL library can be loaded,
 * ORBX_E_NODEVICE without a GPU, ORBX_E_HIP for an RCCL failure (orbx_last_error holds ncclGetErrorString). */
#define ORBX_COMM_ID_BYTES 128
typedef struct orbx_comm orbx_comm;
int orbx_comm_unique_id(uint8_t id[ORBX_COMM_ID_BYTES]);
int orbx_comm_create(const uint8_t id[ORBX_COMM_ID_BYTES], int n_ranks, int rank, int device, orbx_comm** out);
int orbx_comm_adopt(void* nccl_comm, int device, orbx_comm** out);
void orbx_comm_destroy(orbx_comm* c);
int orbx_comm_size(const orbx_comm* c, int* n_ranks, int* rank);
int orbx_allgather_descriptors(orbx_extractor* ex, orbx_comm* c, int n_images, uint8_t* d_all_desc, int32_t* d_all_counts);
/* ORDERING RULE: one communicator per rank may (and should) serve every handle of that rank.  RCCL matches a communicator's
 * collectives by issue order, so every rank must make the same orbx_allgather_descriptors calls in the same order; the calls of
 * one communicator are chained on the device (each waits, stream-side, for the previous one's completion event), so handles
 * on different streams never run two collectives of the communicator concurrently.  orbx_comm_wait blocks the HOST until the
 * communicator's most recent collective has completed, at most timeout_ms: ORBX_OK, or ORBX_E_TIMEOUT with a message that
 * names the collective's sequence number and the likely causes -- a bounded wait in place of a hang in orbx_sync when a
 * rank is missing or out of order.  n_collectives (optional) receives the number of collectives enqueued so far. */
int orbx_comm_wait(orbx_comm* c, int timeout_ms, unsigned long long* n_collectives);

/* Device-resident results of the last (batch) extraction: keypoints [n_images][cap] and descriptors
 * [n_images][cap][32], counts[n_images] (n) and mono[n_images] (monoIndex), all on the device. */
int orbx_batch_results_device(const orbx_extractor* ex, const orbx_keypoint** d_kps, const uint8_t** d_desc,
                              const int32_t** d_counts, const int32_t** d_mono, int* cap);
/* Copy one image's results to the host (synchronises the handle's stream). Returns monoIndex or error. */
int orbx_batch_download(orbx_extractor* ex, int image, orbx_keypoint* kps, uint8_t* desc, int cap, int* n_out);

/* Replaces reads of the public member ORBextractor::mvImagePyramid (include/ORBextractor.h:86;
 * used by src/Frame.cc:927,1011,1024,1029): copies level `level` of image `image` of the last extraction
 * to dst (dst_stride bytes per row; dst may be NULL to query the size only). blurred != 0 returns the
 * 7x7 Gaussian-blurred working copy (src/ORBextractor.cc:1074-1076) instead (computed on demand, once per extraction).
 * Lifetime: level 0 of a batch extracted with orbx_extract_batch_device IS the caller's device buffer (never copied), so
 * reading level 0 -- plain or blurred -- requires that buffer to be alive and unchanged; levels >= 1 and every level of the
 * host entry points (orbx_extract, orbx_extract_stereo, orbx_extract_batch) live in handle-owned memory until the next
 * extraction on the handle. */
int orbx_pyramid_level(orbx_extractor* ex, int image, int level, int blurred, uint8_t* dst,
                       ptrdiff_t dst_stride, int* w, int* h);
/* All (n_levels <= nlevels) levels of one image of the last extraction into caller buffers with ONE synchronisation:
 * dst[l] receives level l (w_l x h_l bytes, rows dst_stride[l] apart; NULL entries are skipped); the copies are queued
 * asynchronously on the handle's stream and the call returns after a single stream synchronisation.  This is what the C++
 * mirror's mvImagePyramid refresh uses (one call per eye instead of 2 x nlevels blocking copies).
 * Level 0 of a batch extracted with orbx_extract_batch_device is the CALLER's device buffer: it must still be alive. */
int orbx_pyramid_download(orbx_extractor* ex, int image, int n_levels, uint8_t* const* dst, const ptrdiff_t* dst_stride);
/* The reference keeps its pyramid in host memory and an UNMODIFIED Frame::ComputeStereoMatches reads it there
 * (`mpORBextractorLeft->mvImagePyramid[l]`, src/Frame.cc:927,1011,1024,1029; include/ORBextractor.h:86).
 * orbx_set_host_pyramid(handle, 1) makes the single-frame host entries (orbx_extract, orbx_extract_stereo) keep such a
 * host copy current: every level of their image(s) is copied into page-locked memory owned by the handle, by the DMA
 * engines on a side stream BESIDE the frame's kernels (orbx_extract_stereo: from the moment both pyramids exist), and the
 * call returns after both.  orbx_host_pyramid_level then hands out the level in place -- pointer, size and row stride,
 * exactly what a `cv::Mat(h, w, CV_8UC1, data, stride)` header needs -- with no further copy and no synchronisation.
 * Lifetime = the reference's: until the next extraction on the handle (src/ORBextractor.cc:1108-1145 overwrites
 * mvImagePyramid on every call).  image = 0 (orbx_extract; the left eye) or 1 (the right eye of orbx_extract_stereo). */
int orbx_set_host_pyramid(orbx_extractor* ex, int enable);
int orbx_host_pyramid_level(const orbx_extractor* ex, int image, int level, const uint8_t** data, int* w, int* h,
                            ptrdiff_t* stride);

/* Stage taps for differential tests: FAST candidates handed to DistributeOctTree for (image, level), in
 * unspecified order (x, y relative to the (16,16) window origin as in src/ORBextractor.cc:965-967;
 * response = FAST score).  Returns the count or a negative error; copies at most cap entries. */
int orbx_debug_candidates(orbx_extractor* ex, int image, int level, int32_t* xys, int cap);
/* k_octree alone on the caller's candidates (tests/test_octree_rules.py): DistributeOctTree of n_images images of width x height,
 * every level, with the launch an extraction of that batch makes -- the plan's launch for batches above two images, 512 threads
 * otherwise, under orbx_debug_set_octree_class / orbx_debug_set_octree_global.  No pyramid, no FAST: the candidates are written
 * into k_detect's per-cell store in the FAST cell each belongs to (cell = (y - 3) / hCell, (x - 3) / wCell), in the caller's
 * order inside a cell -- ties between equal responses are broken by (cell row, cell column, y, x), never by that order.
 *   counts[image * nlevels + level]   candidates of the (image, level)
 *   xyr                               their (x, y, response) triples back to back, image-major, then level; x, y relative to
 *                                     the (16,16) window origin as orbx_debug_candidates returns them
 *   sel_counts[image * nlevels + level], sel[((image * nlevels + level) * sel_cap + i) * 3 ..]   the selected keys in list
 *                                     order as (x, y, response), x, y in level coordinates
 * Sets the handle's geometry and image count like an extraction (orbx_debug_candidates and orbx_level_stats work afterwards;
 * pyramid, keypoints and descriptors of the handle are NOT those of this call).  ORBX_E_CAPACITY when a level selects more than
 * sel_cap keys.  Everything orbx_debug_octree_check rejects is rejected here before anything is written or launched. */
int orbx_debug_octree(orbx_extractor* ex, int width, int height, int n_images, const int32_t* counts, const int32_t* xyr,
                      int32_t* sel_counts, int32_t* sel, int sel_cap);
/* The argument check of orbx_debug_octree (host only, no device), for an extractor of parameters p: ORBX_E_BADARG for a
 * coordinate outside the level's detectable window (3 <= x < 3 + min(W - 6, nCols * wCell) with W = level width - 32, likewise
 * y), a response outside 1 .. 255, a pixel given twice, a FAST cell with more candidates than its slots (cellCap), a level with
 * more than its dense list holds (candCap) -- no crafted input makes the kernel index outside its tables. */
int orbx_debug_octree_check(const orbx_params* p, int width, int height, int n_images, const int32_t* counts, const int32_t* xyr);

/* ---- ORBmatcher / Frame matching -------------------------------------------------------------------- */

/* Replaces ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1959-1973) — host-side convenience, the
 * device matchers use v_bcnt on the same 8 little-endian words. */
int orbx_hamming256(const void* a, const void* b);

/* Replaces Frame::ComputeStereoMatches (src/Frame.cc:921-1084) for n_pairs rectified pairs whose left
 * images are images [first_left, first_left+n_pairs) of `left`'s last extraction and whose right images are
 * [first_right, ...) of `right`'s (left == right is allowed: one handle holding both eyes).  bf = mbf,
 * b = mb (maxD = bf / b).  Results stay on the device of `left`:
 * uRight / depth [n_pairs][cap_left] floats (-1 = no match).  Enqueued on left's stream after right's work. */
int orbx_stereo_match_batch(orbx_extractor* left, int first_left, orbx_extractor* right, int first_right,
                            int n_pairs, float bf, float b);
int orbx_stereo_results_device(const orbx_extractor* left, const float** d_uright, const float** d_depth);
/* Host copy of pair `pair` (synchronises): min(cap, cap_left) entries of each row.  The association (and the RGB-D lookup)
 * writes the entries of the left image's keypoints; the rows past that count are neither read nor written -- they hold what
 * the buffer held before, from an earlier and larger frame for instance -- and only entries [0, count) are results. */
int orbx_stereo_download(orbx_extractor* left, int pair, float* uright, float* depth, int cap);

/* ---- RGB-D frames ----------------------------------------------------------------------------------------------------------
 * Depth image types: OpenCV's CV_16U and CV_32F (single channel).  Any other type is ORBX_E_UNSUPPORTED. */
#define ORBX_DEPTH_U16 2
#define ORBX_DEPTH_F32 5
/* Replaces Frame::ComputeStereoFromRGBD (src/Frame.cc:1086-1104) -- with Tracking::GrabImageRGBD's depth conversion
 * (src/Tracking.cc:1490-1547) folded in -- for n_frames device-resident depth images: frame f is image first_image + f of ex's
 * last extraction, its depth image (depth_type, the size of that extraction, rows row_pitch bytes apart) starts at
 * d_depth + f * image_pitch; base and pitches are multiples of the element size.  depth_scale = Tracking::mDepthMapFactor
 * (1 / RGBD.DepthMapFactor, or 1 when |factor| < 1e-5: src/Tracking.cc:610-614); the library applies the reference's skip
 * rule itself (a CV_32F image with |depth_scale - 1| <= 1e-5 is used unscaled; every other image is scaled by one float
 * multiply per read pixel).  Per keypoint i: d = depth at row (int)mvKeys[i].pt.y, column (int)mvKeys[i].pt.x (the DISTORTED
 * point); d > 0 gives mvDepth = d and mvuRight = mvKeysUn[i].pt.x - bf / d (bf = mbf), anything else (0, negative, -0, NaN,
 * and points whose truncated coordinates fall outside the image) gives -1 for both.  mvKeysUn is computed inside the kernel
 * (Frame::UndistortKeyPoints, src/Frame.cc:853-885: K = fx fy cx cy, dist = mDistCoef, n_dist <= 14 with terms 12, 13 zero; K may be NULL when
 * n_dist == 0 or dist[0] == 0, where mvKeysUn = mvKeys); d_kps_un, a caller-owned DEVICE array [n_frames][cap] (cap =
 * orbx_batch_results_device's), receives it when not NULL.
 * The results land in the handle's stereo result arrays: pair f = frame f, so orbx_stereo_results_device,
 * orbx_stereo_download, orbx_batch_download_async(..., n_pairs <= n_frames) and every batched matcher's stereo_pair0 read
 * them as they read ComputeStereoMatches' results; rows past a frame's keypoint count are left untouched, as the stereo
 * association leaves them.  The next extraction invalidates them.  Enqueued on the handle's stream, no synchronisation: the
 * depth images must stay valid until orbx_sync. */
int orbx_rgbd_depth_batch(orbx_extractor* ex, int first_image, int n_frames, const void* d_depth, int depth_type,
                          ptrdiff_t row_pitch, ptrdiff_t image_pitch, float depth_scale, float bf, const float K[4],
                          const float* dist, int n_dist, orbx_keypoint* d_kps_un);
/* ONE RGB-D frame with one synchronisation: replaces the RGB-D Frame constructor's ExtractORB(0, imGray, 0, 0);
 * UndistortKeyPoints(); ComputeStereoFromRGBD(imDepth) (src/Frame.cc:281-348) and GrabImageRGBD's depth conversion.  The
 * extraction is orbx_extract's (kps / desc / cap / n_out / return value as there, lapping area {0, 0}; *mono receives
 * monoIndex); mvKeysUn is computed on the device from the handle's keypoints and travels back in the same result gather.
 * The depth lookup runs on the HOST, from the caller's host depth image (depth_type, w x h, rows depth_stride bytes apart)
 * with the rule of orbx_rgbd_depth_batch: the frame reads ~N pixels of a depth image the Frame never keeps, and uploading
 * the whole image (1.8 MB at 1280x720 u16) would cost about as much as the extraction, where reading N pixels on the host
 * costs microseconds.  Any of kps, desc, kps_un, uright, depth_out may be NULL; orbx_host_results(ex, 0, ...) hands out
 * keypoints, descriptors, uright and depth in place afterwards, as after orbx_extract_stereo.  Returns monoIndex (>= 0),
 * ORBX_E_EMPTY for an empty image, or another negative error. */
int orbx_extract_rgbd(orbx_extractor* ex, const uint8_t* img, int w, int h, ptrdiff_t stride, const void* depth,
                      int depth_type, ptrdiff_t depth_stride, float depth_scale, float bf, const float K[4], const float* dist,
                      int n_dist, orbx_keypoint* kps, uint8_t* desc, int cap, int* n_out, int* mono, orbx_keypoint* kps_un,
                      float* uright, float* depth_out);

/* Replaces cv::BFMatcher(NORM_HAMMING).knnMatch(Q, T, k=2) + Lowe ratio of
 * Frame::ComputeStereoFishEyeMatches (src/Frame.cc:46,1293-1302).  Host descriptor rows in, host results
 * out: idx2 / dist2 [nQ][2] (-1 when the train set has fewer rows), ratio_ok[nQ] = d0 < d1*0.7. */
int orbx_bf_knn2(int device, const uint8_t* descQ, int nQ, const uint8_t* descT, int nT, int32_t* idx2,
                 int32_t* dist2, uint8_t* ratio_ok);

/* The fisheye stereo rig Frame::ComputeStereoFishEyeMatches works on: the two KannalaBrandt8 cameras
 * (GeometricCamera::mvParameters = fx fy cx cy k0 k1 k2 k3, include/CameraModels/KannalaBrandt8.h:42-57), the Newton
 * stop of KannalaBrandt8::unproject (`precision`, :102) and the left-from-right transform mRlr / mtlr
 * (include/Frame.h:208-209, src/Frame.cc:1240-1243), R12 row-major. */
typedef struct orbx_kb8_rig {
  float cam1[8];
  float cam2[8];
  float precision;
  float R12[9];
  float t12[3];
} orbx_kb8_rig;

/* Replaces the whole of Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1273-1331): brute-force 2-NN of the
 * lapping-area rows [mono_left, n_left) x [mono_right, n_right) (as orbx_bf_knn2), Lowe ratio 0.7, and for every
 * surviving pair KannalaBrandt8::TriangulateMatches (src/CameraModels/KannalaBrandt8.cpp:341-432: unproject by Newton
 * iteration, parallax gate 0.9998, linear triangulation = smallest right singular vector of the 4x4 system, cheirality
 * and the two chi-square reprojection gates 5.991 * mvLevelSigma2[octave]).  Outputs (host, caller-allocated):
 * left_to_right[n_left] = mvLeftToRightMatch, right_to_left[n_right] = mvRightToLeftMatch (serial semantics: a right
 * keypoint claimed by several left ones keeps the LAST), depth[n_left] = mvDepth (-1 = none), points3d[n_left][3] =
 * mvStereo3Dpoints (zeros where unmatched), *n_desc_matches = pairs that passed the ratio test (may be NULL).
 * Returns nMatches >= 0 or an ORBX_E_* code.  This is the one floating-point routine of the path: results agree with
 * the reference to float rounding (device libm, no Eigen), not bit for bit -- see DESIGN.md. */
int orbx_fisheye_stereo_match(int device, const orbx_keypoint* kps_left, const uint8_t* desc_left, int n_left,
                              int mono_left, const orbx_keypoint* kps_right, const uint8_t* desc_right, int n_right,
                              int mono_right, const orbx_kb8_rig* rig, const float* level_sigma2, int n_levels,
                              int32_t* left_to_right, int32_t* right_to_left, float* depth, float* points3d,
                              int32_t* n_desc_matches);

/* The same routine on device-resident extraction results (config C4, batched many-camera mode): pair p associates
 * image first_left + p of `left`'s last extraction with image first_right + p of `right`'s (left == right allowed);
 * the lapping rows [monoIndex, n) and mvLevelSigma2 come from the handles.  Enqueued on left's stream after right's
 * work; results stay on the device of `left`: left_to_right / depth [n_pairs][cap_left], points3d [n_pairs][cap_left][3],
 * right_to_left [n_pairs][cap_right], counts [n_pairs][2] = {nMatches, descMatches}. */
int orbx_fisheye_stereo_match_batch(orbx_extractor* left, int first_left, orbx_extractor* right, int first_right,
                                    int n_pairs, const orbx_kb8_rig* rig);
int orbx_fisheye_results_device(const orbx_extractor* left, const int32_t** d_left_to_right,
                                const int32_t** d_right_to_left, const float** d_depth, const float** d_points3d,
                                const int32_t** d_counts);
/* Host copy of pair `pair` (synchronises; any pointer may be NULL).  Returns nMatches or a negative error. */
int orbx_fisheye_download(orbx_extractor* left, int pair, int32_t* left_to_right, int32_t* right_to_left, float* depth,
                          float* points3d, int cap_left, int cap_right, int32_t* n_desc_matches);

/* ---- image pre-processing in front of the extractor ------------------------------------------ */

/* Replaces cv::cvtColor(im, im, cv::COLOR_{RGB,BGR,RGBA,BGRA}2GRAY) of Tracking::GrabImageStereo / RGBD / Monocular
 * (src/Tracking.cc:1394-1412, 1441-1459, 1481-1499): OpenCV's 8-bit fixed-point formula, coefficients 9798 / 19235 /
 * 3735 with (sum + 16384) >> 15.  channels = 3 or 4 (interleaved), rgb_order != 0 when the first channel is red (mbRGB).
 * Host images in and out. */
int orbx_cvt_gray(int device, const uint8_t* src, int w, int h, ptrdiff_t src_stride, int channels, int rgb_order,
                  uint8_t* dst, ptrdiff_t dst_stride);
/* Replaces cv::resize(im, out, newImSize) (INTER_LINEAR) of System::TrackStereo / TrackRGBD / TrackMonocular
 * (src/System.cc:297-298, 369-370, 437-438) for 8UC1 / 8UC3 / 8UC4 images: the fixed-point bilinear arithmetic of
 * ComputePyramid's cv::resize on every interleaved channel. */
int orbx_resize_linear(int device, const uint8_t* src, int w, int h, ptrdiff_t src_stride, int channels, uint8_t* dst,
                       int dst_w, int dst_h, ptrdiff_t dst_stride);

/* Replaces cv::remap(im, imToFeed, M1, M2, cv::INTER_LINEAR) of System::TrackStereo (src/System.cc:294-295) with the
 * CV_32F maps Settings::precomputeRectificationMaps builds (src/Settings.cc:557-572): OpenCV's fixed-point bilinear remap
 * (positions rounded to 1/32 px, 15-bit weights, BORDER_CONSTANT 0) on 8UC1 / 8UC3 / 8UC4.  map_x / map_y hold dst_h rows of
 * dst_w floats, map_stride floats apart.  Host images in and out. */
int orbx_remap_linear(int device, const uint8_t* src, int w, int h, ptrdiff_t src_stride, int channels, const float* map_x,
                      const float* map_y, ptrdiff_t map_stride, uint8_t* dst, int dst_w, int dst_h, ptrdiff_t dst_stride);
/* Replaces cv::createCLAHE(clip_limit, cv::Size(tiles_x, tiles_y))->apply(im, im) of the TUM-VI front ends
 * (Examples/Stereo/stereo_tum_vi.cc:100,142-143; Examples/Stereo-Inertial/stereo_inertial_tum_vi.cc:151,190-191; the
 * examples pass 3.0 and 8 x 8) on 8UC1.  Host images in and out (src == dst is allowed). */
int orbx_clahe(int device, const uint8_t* src, int w, int h, ptrdiff_t src_stride, double clip_limit, int tiles_x, int tiles_y,
               uint8_t* dst, ptrdiff_t dst_stride);

/* Device-resident pre-processing chain in front of the extractor, so that raw camera frames never return to the host:
 * [CLAHE] -> [remap | resize] -> [gray], the order in which the reference applies them (example main: clahe->apply;
 * System::TrackStereo: remap or resize, src/System.cc:288-302; Tracking::GrabImageStereo: cvtColor, src/Tracking.cc:1394-1412).
 * A stage is enabled by its fields: clahe_tiles_x/y > 0 (single-channel frames only); map_x/map_y != NULL (n_maps maps of
 * out_h x out_w floats each, map m directly after map m-1, rows map_stride floats apart, 0 = out_w; frame i of a batch uses
 * map i % n_maps, i.e. 2 maps = left / right eye interleaved); otherwise out_w x out_h != src size enables cv::resize;
 * channels 3 / 4 enables the gray conversion.  The maps are copied to the device at creation. */
typedef struct orbx_preproc_params {
  int32_t src_w, src_h, channels, rgb_order;
  int32_t out_w, out_h;
  const float* map_x;
  const float* map_y;
  ptrdiff_t map_stride;
  int32_t n_maps;
  double clahe_clip_limit;
  int32_t clahe_tiles_x, clahe_tiles_y;
} orbx_preproc_params;
typedef struct orbx_preproc orbx_preproc;
int orbx_preproc_create(const orbx_preproc_params* p, int max_batch, int device, orbx_preproc** out);
void orbx_preproc_destroy(orbx_preproc* pp);
int orbx_preproc_output_size(const orbx_preproc* pp, int* out_w, int* out_h);
/* One host frame through the chain (map `map_index`), host result out_w x out_h gray. */
int orbx_preproc_run(orbx_preproc* pp, const uint8_t* frame, ptrdiff_t stride, int map_index, uint8_t* dst, ptrdiff_t dst_stride);
/* n_frames device-resident raw frames (frame i at d_frames + i*image_pitch) through the chain; synchronises and returns the
 * device-resident result (owned by the handle, valid until its next run). */
int orbx_preproc_run_device(orbx_preproc* pp, const uint8_t* d_frames, int n_frames, ptrdiff_t row_pitch,
                            ptrdiff_t image_pitch, const uint8_t** d_out, int* out_w, int* out_h, ptrdiff_t* out_row_pitch,
                            ptrdiff_t* out_image_pitch);
/* orbx_extract_batch_device on raw frames: the chain and the extraction are enqueued on the extractor's stream, nothing
 * synchronises.  The pre-processor's buffers back level 0 of the pyramid until orbx_sync: use one orbx_preproc per extractor
 * handle in flight. */
int orbx_extract_batch_raw_device(orbx_extractor* ex, orbx_preproc* pp, const uint8_t* d_frames, int n_frames,
                                  ptrdiff_t row_pitch, ptrdiff_t image_pitch, const int32_t* lap);

/* ---- bag of words --------------------------------------------------------------------------------- */

/* Replaces ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (include/ORBVocabulary.h;
 * Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h) as far as Frame::ComputeBoW uses it: the tree on the device.
 * orbx_vocabulary_load_text replaces loadFromTextFile(strVocFile) of System::System (src/System.cc:131,
 * TemplatedVocabulary.h:1338-1421; "k L scoring weighting", then one node per line: parent isLeaf 32 bytes weight).
 * orbx_vocabulary_create takes the same columns: node 0 = root (its columns are ignored), parent[i] < i, the children of a
 * node in file order, words numbered in the file order of the leaves.  info = k, L, n_nodes, n_words, scoring, weighting. */
typedef struct orbx_vocabulary orbx_vocabulary;
int orbx_vocabulary_create(int device, int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                           const uint8_t* is_leaf, const uint8_t* descriptors, const double* weights, orbx_vocabulary** out);
int orbx_vocabulary_load_text(int device, const char* path, orbx_vocabulary** out);
void orbx_vocabulary_destroy(orbx_vocabulary* voc);
int orbx_vocabulary_info(const orbx_vocabulary* voc, int32_t info[6]);

/* Replaces Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:846-851, src/KeyFrame.cc:100-107):
 * mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4) (TemplatedVocabulary.h:1125-1250) for n descriptors (n x 32
 * bytes, n <= 8192).  mBowVec: n_words ascending (word id, value) pairs, values bit-identical to the reference's sequential
 * double additions and normalisation; mFeatVec as CSR: n_nodes ascending node ids, features of node j =
 * feature_idx[node_start[j] .. node_start[j + 1]) in ascending order.  Output arrays hold n entries (node_start n + 1).
 * Returns the number of features in the feature vector (stopped words are left out) or a negative error. */
int orbx_bow_transform(const orbx_vocabulary* voc, const uint8_t* desc, int n, int levelsup, uint32_t* word_ids,
                       double* word_values, int* n_words, uint32_t* node_ids, int32_t* node_start, uint32_t* feature_idx,
                       int* n_nodes);
/* The same for every image of the handle's last extraction, enqueued on its stream; results stay on the device: arrays of
 * [n_images][cap] (node_start [n_images][cap + 1]), counts [n_images][3] = n_words, n_nodes, n_features. */
int orbx_bow_transform_batch(orbx_extractor* ex, const orbx_vocabulary* voc, int levelsup);
int orbx_bow_results_device(const orbx_extractor* ex, const uint32_t** d_word_ids, const double** d_word_values,
                            const uint32_t** d_node_ids, const int32_t** d_node_start, const uint32_t** d_feature_idx,
                            const int32_t** d_counts, int* cap);
/* Host copy of image `image` (synchronises); cap = capacity of the arrays.  Returns n_features or a negative error. */
int orbx_bow_download(orbx_extractor* ex, int image, uint32_t* word_ids, double* word_values, int* n_words, uint32_t* node_ids,
                      int32_t* node_start, uint32_t* feature_idx, int* n_nodes, int cap);

/* Replaces ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)
 * (src/ORBmatcher.cc:230-404).  kf_* = pKF->mFeatVec (CSR as above), its keypoints (angle is read; left | right
 * concatenated for two-camera rigs), mDescriptors and kf_valid[i] = (vpMapPointsKF[i] && !isBad()); f_* = F.mFeatVec,
 * F's keypoints and descriptors, n_left_f = F.Nleft (-1 for monocular / rectified frames).  matches[i] = index of the
 * keyframe feature whose map point F's feature i received, or -1 (vpMapPointMatches).  nnratio = mfNNratio,
 * check_orientation = mbCheckOrientation.  Returns nmatches or a negative error.
 * Limit: a vocabulary node that both feature vectors contain may hold at most 4096 features of F (their "already matched"
 * marks are kept on chip; a node of ORBvoc.txt at levelsup 4 holds about 15 of a 1500-feature frame).  A larger one is refused
 * with ORBX_E_UNSUPPORTED -- there is no slower path -- and every entry of matches is then -1.  A node of any size that
 * pKF does not have is never looked at.  pKF's side of a node has no limit. */
int orbx_search_by_bow(int device, const uint32_t* kf_node_ids, const int32_t* kf_node_start, const uint32_t* kf_feature_idx,
                       int n_kf_nodes, const orbx_keypoint* kf_kps, const uint8_t* kf_desc, const uint8_t* kf_valid, int n_kf,
                       const uint32_t* f_node_ids, const int32_t* f_node_start, const uint32_t* f_feature_idx, int n_f_nodes,
                       const orbx_keypoint* f_kps, const uint8_t* f_desc, int n_f, int n_left_f, float nnratio,
                       int check_orientation, int32_t* matches);
/* The same search for the frames of an extraction BATCH: frame f = image first_image + f of `ex`'s last batch, whose keypoints,
 * descriptors and feature vector (orbx_bow_transform_batch must have run on that extraction) stay in HBM; the key frame of pair f
 * comes from the host as strided arrays -- kf_node_ids [n_frames][nodes_stride], kf_node_start [n_frames][nodes_stride + 1],
 * kf_feature_idx / kf_kps / kf_desc / kf_valid [n_frames][kf_stride](x 32) with n_kf_nodes[f] / n_kf[f] valid entries.
 * matches is [n_frames][cap] (cap = orbx_batch_results_device's cap; -1 past a frame's keypoints), n_matches [n_frames].
 * Every kernel runs ONCE for all pairs (blockIdx.y = pair); results are those of n_frames separate calls.
 * Returns the total number of matches or a negative error.  The limit of 4096 frame features per shared vocabulary node holds
 * for every pair: if one pair exceeds it the call returns ORBX_E_UNSUPPORTED, every entry of matches (all pairs) is -1 and
 * n_matches[f] is -1 for the pairs over the limit and 0 for the others. */
int orbx_search_by_bow_batch(orbx_extractor* ex, int first_image, int n_frames, const uint32_t* kf_node_ids,
                             const int32_t* kf_node_start, const int32_t* n_kf_nodes, int nodes_stride,
                             const uint32_t* kf_feature_idx, const orbx_keypoint* kf_kps, const uint8_t* kf_desc,
                             const uint8_t* kf_valid, const int32_t* n_kf, int kf_stride, int n_left_f, float nnratio,
                             int check_orientation, int32_t* matches, int32_t* n_matches);

/* Replaces Frame::UndistortKeyPoints (src/Frame.cc:853-885): mvKeysUn from mvKeys through
 * cv::undistortPoints(mat, mat, K, mDistCoef, cv::Mat(), mK) -- five fixed-point iterations of the inverse distortion
 * in double, then x' = fx x + cx.  K = fx fy cx cy (Pinhole::toK()); dist = the n_dist (4, 5, 8, 12 or 14) OpenCV
 * coefficients of mDistCoef, tilt terms unsupported (must be 0).  dist[0] == 0 copies the keypoints, as the reference
 * does.  Host arrays in and out; out may alias kps. */
int orbx_undistort_keypoints(int device, const orbx_keypoint* kps, int n, const float K[4], const float* dist, int n_dist,
                             orbx_keypoint* out);
/* Replaces Frame::ComputeImageBounds (src/Frame.cc:887-919): bounds = mnMinX, mnMinY, mnMaxX, mnMaxY of a cols x rows
 * image (the undistorted corners, or 0, 0, cols, rows when dist[0] == 0). */
int orbx_compute_image_bounds(int device, int cols, int rows, const float K[4], const float* dist, int n_dist,
                              float bounds[4]);

/* Replaces ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:618-764) incl. Frame::GetFeaturesInArea /
 * AssignFeaturesToGrid / PosInGrid on F2 (src/Frame.cc:520-547,765-844) and ComputeThreeMaxima
 * (src/ORBmatcher.cc:1920-1955).  kps are the undistorted keypoints (mvKeysUn); bounds = mnMinX, mnMinY,
 * mnMaxX, mnMaxY of F2; prev_matched = vbPrevMatched (2*n1 floats, in/out); matches12 = vnMatches12 (n1).
 * Returns nmatches or a negative error. */
int orbx_search_for_initialization(int device, const orbx_keypoint* kps1, const uint8_t* desc1, int n1,
                                   const orbx_keypoint* kps2, const uint8_t* desc2, int n2, float min_x,
                                   float min_y, float max_x, float max_y, float* prev_matched,
                                   int32_t* matches12, int window_size, float nnratio, int check_orientation);
/* The same search for the frames of an extraction BATCH (many-camera mode: every camera still initialising its map matches its
 * initial frame against its current one, src/Tracking.cc:2438-2440, in one call).  Pair f: F2 = image first_image + f of `ex`'s
 * last batch (keypoints taken as mvKeysUn and descriptors stay in HBM), F1 = kps1 / desc1 [f * stride .. f * stride + n1[f]) on
 * the host; prev_matched is [n_frames][stride][2] (in/out), matches12 [n_frames][stride], n_matches [n_frames].  Every kernel
 * of the chain runs ONCE for all pairs (blockIdx.y = pair) with a fixed number of fixed-point rounds enqueued without reading
 * a convergence flag; a pair that needs more rounds or larger candidate lists is redone through the one-shot call: results are
 * those of n_frames separate orbx_search_for_initialization calls.  Returns the total number of matches or a negative error. */
int orbx_search_for_initialization_batch(orbx_extractor* ex, int first_image, int n_frames, const orbx_keypoint* kps1,
                                         const uint8_t* desc1, const int32_t* n1, int stride, float min_x, float min_y,
                                         float max_x, float max_y, float* prev_matched, int32_t* matches12, int window_size,
                                         float nnratio, int check_orientation, int32_t* n_matches);

/* Replaces Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cc:520-547,833-844: 64 x 48 grid, round-to-cell) and
 * Frame::GetFeaturesInArea (src/Frame.cc:765-831) for a batch of queries.  kps = mvKeysUn (n), bounds = mnMinX/Y,
 * mnMaxX/Y; queries = n_queries x {x, y, r, minLevel, maxLevel} floats.  Output is CSR: offsets[n_queries + 1] and
 * indices (keypoint indices in the reference's order: ix outer, iy inner, in-cell ascending).  Optionally returns
 * the grid itself: grid_cell_start[64*48 + 1] (cell ix*48 + iy) and grid_items[n] (= mGrid[ix][iy] concatenated).
 * Returns the total number of indices or a negative error (ORBX_E_CAPACITY if indices_cap is too small; offsets are
 * still valid then). */
int orbx_features_in_area(int device, const orbx_keypoint* kps, int n, float min_x, float min_y, float max_x,
                          float max_y, const float* queries, int n_queries, int32_t* offsets, int32_t* indices,
                          int indices_cap, int32_t* grid_cell_start, int32_t* grid_items);

/* ---- widening row f1: projection-guided matching ------------------------------------------ */

/* The MapPoint members ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, ...) reads
 * (src/ORBmatcher.cc:41-221): mTrackProjX/Y/XR, mTrackViewCos, mTrackDepth, mnTrackScaleLevel, mbTrackInView,
 * isBad(), Observations() > 0, GetDescriptor().  60 bytes. */
typedef struct orbx_map_point_view {
  float proj_x, proj_y, proj_xr, view_cos, track_depth;
  int32_t predicted_level;
  uint8_t in_view, bad, has_observations, pad_;
  uint8_t desc[32];
} orbx_map_point_view;

/* Replaces ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, th, bFarPoints,
 * thFarPoints) (src/ORBmatcher.cc:41-221) for the pinhole case (F.Nleft == -1), serial iMP semantics.
 * F is given by mvKeysUn (n), mDescriptors, mvuRight (may be NULL), the grid bounds mnMinX/Y, mnMaxX/Y and
 * mvScaleFactors (nlevels).  occupied[i] != 0 <=> F.mvpMapPoints[i] already holds a point with Observations() > 0
 * (in/out).  match[i] receives the index of the map point newly assigned to keypoint i, or -1.
 * Returns nmatches or a negative error. */
int orbx_search_by_projection(int device, const orbx_keypoint* kps_un, const uint8_t* desc, const float* u_right,
                              int n, float min_x, float min_y, float max_x, float max_y, const float* scale_factors,
                              int nlevels, const orbx_map_point_view* map_points, int n_map_points, float th,
                              int far_points, float th_far_points, float nnratio, uint8_t* occupied, int32_t* match);

/* One LastFrame point after the reference's pose / camera projection (src/ORBmatcher.cc:1606-1648): uv, the
 * right-image coordinate ur = u - mbf * invz, radius = th * mvScaleFactors[nLastOctave], the level window picked by
 * bForward / bBackward ((nLastOctave, -1), (0, nLastOctave) or (nLastOctave-1, nLastOctave+1)), the last-frame
 * keypoint angle, the MapPoint's descriptor and Observations() > 0.  valid = 0 for points the reference skips
 * (no MapPoint, outlier, invz < 0, projection outside the image).  64 bytes. */
typedef struct orbx_projected_point {
  float u, v, ur, radius, angle;
  int32_t min_level, max_level;
  uint8_t valid, has_observations, pad_[2];
  uint8_t desc[32];
} orbx_projected_point;

/* Replaces the matching part of ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th,
 * bMono) (src/ORBmatcher.cc:1594-1806, pinhole case): window search on CurrentFrame's grid, occupancy gate,
 * stereo-consistency gate, best Hamming <= TH_HIGH, assignment in serial order, rotation-histogram cull
 * (check_orientation).  match[i2] = LastFrame point index assigned to keypoint i2 or -1.  Returns nmatches. */
int orbx_search_by_projection_frame(int device, const orbx_keypoint* kps_un, const uint8_t* desc, const float* u_right,
                                    int n, float min_x, float min_y, float max_x, float max_y,
                                    const orbx_projected_point* points, int n_points, int check_orientation,
                                    uint8_t* occupied, int32_t* match);

/* The two pinhole SearchByProjection flavours above on the frames of an extraction BATCH (the many-camera mode: one tracking step
 * of n_frames cameras).  Frame f = image first_image + f of `ex`'s last batch: its keypoints (taken as mvKeysUn: pinhole without
 * distortion / rectified input, like the batch itself) and descriptors stay in HBM; points / map points of frame f are
 * points[f * points_stride .. + n_points[f]); bounds = mnMinX .. mnMaxY; scale factors = the handle's; stereo_pair0 >= 0 takes
 * mvuRight of frame f from pair stereo_pair0 + f of the handle's last orbx_stereo_match_batch (-1: monocular, no consistency
 * check); occupied_in (may be NULL = all free) / occupied / match are [n_frames][cap] with cap = orbx_batch_results_device's cap,
 * n_matches [n_frames].  Every kernel of the chain runs ONCE for all frames (blockIdx.y = frame) with a fixed number of
 * fixed-point rounds enqueued blindly; a frame that needs more (or larger candidate lists) is redone through the one-shot path:
 * results are those of n_frames separate calls.  map_points == NULL (round 6): the views come from the handle's last
 * orbx_project_map_points_batch and never touch the host (points_stride and every n_map_points[f] must equal its n); points ==
 * NULL in the frame flavour: from the last orbx_project_last_frames_batch (points_stride / n_points[f] = the upload's).
 * Returns the total number of matches or a negative error. */
int orbx_search_by_projection_batch(orbx_extractor* ex, int first_image, int n_frames, float min_x, float min_y, float max_x,
                                    float max_y, const orbx_map_point_view* map_points, const int32_t* n_map_points,
                                    int points_stride, float th, int far_points, float th_far_points, float nnratio,
                                    int stereo_pair0, const uint8_t* occupied_in, uint8_t* occupied, int32_t* match,
                                    int32_t* n_matches);
int orbx_search_by_projection_frame_batch(orbx_extractor* ex, int first_image, int n_frames, float min_x, float min_y, float max_x,
                                          float max_y, const orbx_projected_point* points, const int32_t* n_points,
                                          int points_stride, int check_orientation, int stereo_pair0, const uint8_t* occupied_in,
                                          uint8_t* occupied, int32_t* match, int32_t* n_matches);

/* ---- device-side projection for the batched local-map matcher (round 6) -----------------------------------------------------
 * Tracking::SearchLocalPoints (src/Tracking.cc:3303-3328) calls Frame::isInFrustum (src/Frame.cc:632-690) for every local map
 * point, which stores mTrackProjX / Y / XR, mTrackDepth, mnTrackScaleLevel (MapPoint::PredictScale, src/MapPoint.cc:559-573),
 * mTrackViewCos and mbTrackInView in the MapPoint; SearchByProjection then reads them back (src/ORBmatcher.cc:62-76).  Here the
 * local map is uploaded ONCE as structure-of-arrays, every frame of the batch contributes its pose, and the projection, the frustum
 * / distance / viewing-angle gates and the level prediction run on the device: the views never exist on the host.
 * Pose of a pinhole frame = the members isInFrustum reads: mRcw (row-major), mtcw, mOw, the Pinhole parameters fx fy cx cy, mbf. */
typedef struct orbx_frame_pose {
  float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, bf;
} orbx_frame_pose;
/* n local map points: GetWorldPos(), GetNormal() (n x 3 each), mfMinDistance / mfMaxDistance (the 0.8 / 1.2 factors of
 * Get{Min,Max}DistanceInvariance are applied by the library), GetDescriptor() (n x 32), flags bit 0 = isBad(), bit 1 =
 * Observations() > 0.  Copied into the handle; stays valid until the next upload. */
int orbx_map_upload(orbx_extractor* ex, int n, const float* world_pos, const float* normal, const float* min_distance,
                    const float* max_distance, const uint8_t* desc, const uint8_t* flags);
/* isInFrustum(pMP, viewing_cos_limit) of all n uploaded points for n_frames frames (bounds = mnMinX .. mnMaxY); skip (may be NULL)
 * is [n_frames][n], != 0 = the point is not offered to this frame (already matched: mnLastFrameSeen == frame id,
 * src/Tracking.cc:3310-3316).  The views [n_frames][n] stay on the device, attached to the handle, for
 * orbx_search_by_projection_batch(map_points = NULL, points_stride = n, n_map_points[f] = n); views_out (may be NULL) receives
 * a host copy.  Float arithmetic in the reference's expression order; PredictScale's logarithm is the device's logf: a level may
 * differ from a glibc build by one where log(ratio) / logScaleFactor is within rounding of an integer. */
int orbx_project_map_points_batch(orbx_extractor* ex, int n_frames, const orbx_frame_pose* poses, float min_x, float min_y,
                                  float max_x, float max_y, float viewing_cos_limit, const uint8_t* skip,
                                  orbx_map_point_view* views_out);

/* ---- device-side projection for the batched frame-to-frame matcher (round 6) -------------------------------------------------
 * ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) projects LastFrame's map points itself
 * (src/ORBmatcher.cc:1606-1648): x3Dc = Tcw * x3Dw with Tcw a Sophus::SE3f -- the unit-quaternion sandwich of
 * Thirdparty/Sophus/sophus/so3.hpp:358-366 plus the translation --, invzc = 1.0 / z, Pinhole::project, the bounds skips, radius =
 * th * mvScaleFactors[nLastOctave], the level window by bForward / bBackward, ur = u - mbf * invzc.  Here the LastFrames of the
 * batch's cameras are uploaded once per tracking step as structure-of-arrays, every camera contributes its pose, and the
 * orbx_projected_point views are made on the device and stay there for orbx_search_by_projection_frame_batch(points = NULL).
 * Pose = Tcw as Sophus stores it (quaternion x y z w, translation), the Pinhole parameters, mbf and the caller's forward /
 * backward decision (:1611-1612, from tlc(2) and mb): direction 0 = neither, 1 = bForward, 2 = bBackward. */
typedef struct orbx_frame_pose_q {
  float q[4], t[3], fx, fy, cx, cy, bf;
  int32_t direction;
} orbx_frame_pose_q;
/* LastFrame f of camera f (n_frames cameras, points_stride entries each, n_points[f] used): per keypoint i of that LastFrame the
 * world position of mvpMapPoints[i] (n_frames x stride x 3), mvKeys[i].octave, mvKeysUn[i].angle, pMP->GetDescriptor()
 * (x 32), flags bit 0 = the point exists and is no outlier (:1615-1617), bit 1 = Observations() > 0.  Copied into the handle. */
int orbx_last_frames_upload(orbx_extractor* ex, int n_frames, int points_stride, const int32_t* n_points, const float* world_pos,
                            const int32_t* octave, const float* angle, const uint8_t* desc, const uint8_t* flags);
/* The projection block for every uploaded point of n_frames frames (scale factors = the handle's; bounds = mnMinX .. mnMaxY).
 * views_out (may be NULL) receives a host copy [n_frames][points_stride].  Float arithmetic in the reference's expression order
 * (tolerance parity at the gates, like orbx_project_map_points_batch; 0 / 0 projections are marked invalid). */
int orbx_project_last_frames_batch(orbx_extractor* ex, int n_frames, const orbx_frame_pose_q* poses, float min_x, float min_y,
                                   float max_x, float max_y, float th, orbx_projected_point* views_out);

/* Replaces the matching part of the relocalisation matcher ORBmatcher::SearchByProjection(Frame& CurrentFrame,
 * KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1808-1918; callers
 * src/Tracking.cc:3631-3632,3645-3646 with (th, ORBdist) = (10, 100) and (3, 64)).  points[i] = the key frame's i-th
 * map point after the caller's pose / camera projection and gates (:1826-1851): valid = 0 for a missing / bad /
 * already-found point, a projection outside the image bounds or a distance outside the scale-invariance range; (u, v);
 * radius = th * mvScaleFactors[nPredictedLevel]; (min_level, max_level) = (nPredictedLevel - 1, nPredictedLevel + 1);
 * angle = pKF->mvKeysUn[i].angle; desc = pMP->GetDescriptor().  ur and has_observations are not read: this flavour has
 * no stereo gate, and its occupancy gate is a plain non-null test (:1871), so EVERY assignment occupies its keypoint.
 * occupied[i2] != 0 <=> CurrentFrame.mvpMapPoints[i2] != NULL (in/out: on return also set for the new matches and
 * clear again for the ones the rotation-consistency cull removed, :1910-1913).  Best Hamming < 256 by strict first
 * minimum over the free candidates, accepted if <= orb_dist (0..255).  match[i2] = index i of the assigned point or -1.
 * Returns nmatches after the cull, or a negative error.
 * The loop-closing searches SearchByProjection(KeyFrame* pKF, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming) and its
 * vpMatchedKF twin (src/ORBmatcher.cc:406-503, :505-612) run the same loop -- occupancy = vpMatched[idx] != NULL, level window
 * [nPredictedLevel - 1, nPredictedLevel], `bestDist <= TH_LOW * ratioHamming`, no orientation check -- and are served by this
 * entry with (min_level, max_level) = (nPredictedLevel - 1, nPredictedLevel), check_orientation = 0 and
 * orb_dist = floor(TH_LOW * ratioHamming) (tests/test_reloc_triangulation.py checks a literal transcription of that loop). */
int orbx_search_by_projection_keyframe(int device, const orbx_keypoint* kps_un, const uint8_t* desc, int n, float min_x,
                                       float min_y, float max_x, float max_y, const orbx_projected_point* points,
                                       int n_points, int orb_dist, int check_orientation, uint8_t* occupied,
                                       int32_t* match);

/* Replaces ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, vector<pair<size_t, size_t>>& vMatchedPairs,
 * bOnlyStereo, bCoarse) (src/ORBmatcher.cc:886-1106; caller LocalMapping::CreateNewMapPoints) for single-camera key frames
 * (mpCamera2 == NULL in both; NLeft == -1).  *_1 / *_2 = pKF1 / pKF2: mFeatVec as CSR (ascending node ids, as orbx_bow_transform
 * returns it), mvKeysUn, mDescriptors, has_map_point[i] = (GetMapPoint(i) != NULL), u_right = mvuRight (NULL: no stereo
 * observations, i.e. monocular).  scale_factors2 / level_sigma2_2 = pKF2->mvScaleFactors / mvLevelSigma2 (nlevels2 entries);
 * ep = pKF2->mpCamera->project(T2w * pKF1->GetCameraCenter()) (:897-901); F12 = the fundamental matrix
 * Pinhole::epipolarConstrain forms on every call, K1^-T [t12]x R12 K2^-1 (src/CameraModels/Pinhole.cpp:130-133), row-major,
 * computed once by the caller (not read when coarse != 0).  matches12[idx1] = idx2 or -1; vMatchedPairs = its non-negative
 * entries in ascending idx1 (:1095-1103).  Like the reference (vbMatched2 is never set, :933,976) one feature of pKF2 may be
 * paired with several of pKF1.  Returns nmatches after the rotation-consistency cull, or a negative error. */
int orbx_search_for_triangulation(int device, const uint32_t* node_ids1, const int32_t* node_start1, const uint32_t* feature_idx1,
                                  int n_nodes1, const orbx_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_map_point1,
                                  const float* u_right1, int n1, const uint32_t* node_ids2, const int32_t* node_start2,
                                  const uint32_t* feature_idx2, int n_nodes2, const orbx_keypoint* kps2, const uint8_t* desc2,
                                  const uint8_t* has_map_point2, const float* u_right2, int n2, const float* scale_factors2,
                                  const float* level_sigma2_2, int nlevels2, const float ep[2], const float F12[9], int only_stereo,
                                  int coarse, int check_orientation, int32_t* matches12);

/* The two-camera members ORBmatcher::SearchForTriangulation reads when pKF1->mpCamera2 && pKF2->mpCamera2
 * (src/ORBmatcher.cc:906-923, 1007-1042): cam[0..3] = the KannalaBrandt8 mvParameters (fx fy cx cy k0..k3) of pKF1->mpCamera,
 * pKF1->mpCamera2, pKF2->mpCamera, pKF2->mpCamera2; precision = KannalaBrandt8::precision; R[c] / t[c] = rotation (row-major) and
 * translation of Tll = T1w * Tw2, Tlr = T1w * Twr2, Trl = Tr1w * Tw2, Trr = Tr1w * Twr2.  81 floats. */
typedef struct orbx_tri_rig {
  float cam[4][8];
  float precision;
  float R[4][9], t[4][3];
} orbx_tri_rig;

/* ORBmatcher::SearchForTriangulation for two-camera (stereo-fisheye) key frames: kps / desc / has_map_point hold the N = NLeft +
 * NRight features of each key frame (mvKeys then mvKeysRight, n_left = KeyFrame::NLeft); the epipolar test is
 * KannalaBrandt8::epipolarConstrain = TriangulateMatches(...) > 0.0001f (src/CameraModels/KannalaBrandt8.cpp:240-250, :341-417)
 * with (R12, t12, cameras) chosen by the eyes the two features sit in (:1007-1042), sigmaLevel = level_sigma2_1[kp1.octave], unc =
 * level_sigma2_2[kp2.octave]; there is no epipole gate and bStereo is false for every feature, so only_stereo != 0 matches
 * nothing (:957-959).  Float arithmetic in the reference's expression order, the 4x4 null vector by a double one-sided Jacobi
 * instead of Eigen::JacobiSVD<Matrix4f>: accept / reject decisions equal the oracle's unless a gated quantity lies within
 * rounding noise of its threshold (tolerance parity, like orbx_fisheye_stereo_match).  Returns nmatches or a negative error. */
int orbx_search_for_triangulation_rig(int device, const uint32_t* node_ids1, const int32_t* node_start1, const uint32_t* feature_idx1,
                                      int n_nodes1, const orbx_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_map_point1,
                                      int n_left1, int n1, const uint32_t* node_ids2, const int32_t* node_start2,
                                      const uint32_t* feature_idx2, int n_nodes2, const orbx_keypoint* kps2, const uint8_t* desc2,
                                      const uint8_t* has_map_point2, int n_left2, int n2, const float* level_sigma2_1,
                                      const float* level_sigma2_2, int nlevels, const orbx_tri_rig* rig, int only_stereo, int coarse,
                                      int check_orientation, int32_t* matches12);

/* Replaces ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (src/ORBmatcher.cc:766-884;
 * LoopClosing).  *_1 / *_2 = pKF1 / pKF2: mFeatVec as CSR, mvKeysUn (the angle is read), mDescriptors and valid[i] =
 * (vpMapPoints[i] && !vpMapPoints[i]->isBad() && !(NLeft != -1 && i >= mvKeysUn.size())) (:799-806,:817-825).  matches12[idx1] =
 * the feature of pKF2 whose map point vpMatches12[idx1] receives, or -1: per vocabulary node, pKF1's features in list order, best
 * and second best over the partner node's features that are valid and not taken yet (vbMatched2), accepted if bestDist1 < TH_LOW
 * (strict) and bestDist1 < nnratio * bestDist2; then the rotation-consistency cull.  Returns nmatches or a negative error.
 * Limit: a vocabulary node that both key frames contain may hold at most 4096 features of pKF2 (valid or not); a larger one is
 * refused with ORBX_E_UNSUPPORTED and every entry of matches12 is then -1.  pKF1's side of a node has no limit. */
int orbx_search_by_bow_keyframes(int device, const uint32_t* node_ids1, const int32_t* node_start1, const uint32_t* feature_idx1,
                                 int n_nodes1, const orbx_keypoint* kps1, const uint8_t* desc1, const uint8_t* valid1, int n1,
                                 const uint32_t* node_ids2, const int32_t* node_start2, const uint32_t* feature_idx2, int n_nodes2,
                                 const orbx_keypoint* kps2, const uint8_t* desc2, const uint8_t* valid2, int n2, float nnratio,
                                 int check_orientation, int32_t* matches12);

/* One map point of ORBmatcher::Fuse after the reference's projection and gates (src/ORBmatcher.cc:1141-1192: not bad, not already
 * in the key frame, positive depth, inside the image, distance inside the scale-invariance range, viewing angle below 60 degrees):
 * uv, ur = u - mbf * invz, radius = th * mvScaleFactors[nPredictedLevel], nPredictedLevel, GetDescriptor().  valid = 0 for the
 * points the reference skips.  56 bytes. */
typedef struct orbx_fuse_point {
  float u, v, ur, radius;
  int32_t predicted_level;
  uint8_t valid, pad_[3];
  uint8_t desc[32];
} orbx_fuse_point;

/* Replaces the search of ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th, bRight)
 * (src/ORBmatcher.cc:1108-1277; LocalMapping::SearchInNeighbors): per map point KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:
 * 705-749), the level window [nPredictedLevel - 1, nPredictedLevel], the chi-square gate on the reprojection error (5.99
 * monocular, 7.8 with mvuRight[idx] >= 0; float arithmetic as :1217-1237) and the first strict minimum of the descriptor distance
 * (:1195-1256).  kps / desc / u_right = the camera searched: mvKeysUn + mvuRight, or mvKeys / mvKeysRight of a two-camera rig
 * with u_right = NULL (the caller adds NLeft to the indices of the right camera, :1239); bounds = mnMinX .. mnMaxY;
 * inv_level_sigma2 = mvInvLevelSigma2; max_dist = TH_LOW (50).  best_idx[i] = the keypoint point i fuses into (distance <=
 * max_dist) or -1; best_dist[i]
 * (optional) = the minimum over the gated candidates, 256 if there were none.  The Replace / AddObservation / AddMapPoint
 * bookkeeping of a hit (:1259-1271) does not feed back into the search and stays with the caller, in point order.
 * Returns nFused or a negative error.
 * Fuse(KeyFrame* pKF, Sim3f& Scw, vpPoints, th, vpReplacePoint) of loop closing (:1279-1390) runs the same search without the
 * chi-square gate: pass inv_level_sigma2 = 0 for every level (e2 * 0 > 5.99 never holds).
 * ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (:1392-1592) is two such searches -- pKF1's map points in pKF2
 * (:1437-1497) and pKF2's in pKF1 (:1499-1567), no chi-square gate, max_dist = TH_HIGH (100) -- followed by the agreement
 * check vnMatch2[vnMatch1[i1]] == i1 (:1569-1583) on the caller's side (ORB_SLAM3::SearchBySim3 in csrc/ORBmatcher.h). */
int orbx_fuse_search(int device, const orbx_keypoint* kps, const uint8_t* desc, const float* u_right, int n, float min_x,
                     float min_y, float max_x, float max_y, const float* inv_level_sigma2, int nlevels,
                     const orbx_fuse_point* points, int n_points, int max_dist, int32_t* best_idx, int32_t* best_dist);

/* Stereo-fisheye frames (F.Nleft != -1): the frame holds N = n_left + n_right keypoints (mvKeys then mvKeysRight), one
 * descriptor row each in the same order, mGrid over the left and mGridRight over the right keypoints, and the stereo
 * association mvLeftToRightMatch / mvRightToLeftMatch (orbx_fisheye_stereo_match).  orbx_map_point_right carries the
 * right-camera members of MapPoint next to orbx_map_point_view (whose proj_xr is mTrackProjXR): mTrackProjYR,
 * mTrackViewCosR, mnTrackScaleLevelR (-1 = none), mbTrackInViewR. */
typedef struct orbx_map_point_right {
  float proj_yr, view_cos_r;
  int32_t predicted_level_r;
  uint8_t in_view_r, pad_[3];
} orbx_map_point_right;

/* Device-side projection for stereo-fisheye frames (Nleft != -1; the pinhole form is orbx_project_map_points_batch, same uploaded map):
 * Frame::isInFrustum runs isInFrustumChecks (src/Frame.cc:689-697, :1333-1410)
 * once per camera with KannalaBrandt8::project (src/CameraModels/KannalaBrandt8.cpp:67-86).  A camera's pose = the (mR, mt, twc) the
 * reference forms at :1342-1351 -- (mRcw, mtcw, mOw) for the left camera, (Rrl * mRcw, Rrl * mtcw + trl, mRwc * mTlr.translation()
 * + mOw) for the right one, computed by the caller in float -- plus that camera's eight KB8 parameters.  The views of both
 * cameras stay on the device for orbx_search_by_projection_fisheye_batch(map_points = NULL, map_points_right = NULL); views_out /
 * views_right_out (may be NULL) receive host copies in the matcher's input form ([n_frames][n] each).  Tolerance parity (device
 * atan2f / cosf / sinf / logf).
 * track_depth (mTrackDepth, the distance |Pc| in the LEFT camera) is written for points the left camera accepts and is 0 for every
 * other point, also for one that only the right camera sees: the reference leaves mTrackDepth of such a point at whatever an
 * earlier frame wrote (src/Frame.cc:1394-1400 set it in the left branch only), so its bFarPoints gate (src/ORBmatcher.cc:57) reads
 * a stale value there; here the gate never culls a right-only point.  A caller that wants the host-fed behaviour passes its own
 * mTrackDepth through orbx_search_by_projection_fisheye_batch's map_points.  tests/test_projection_device.py pins the 0. */
typedef struct orbx_frame_pose_kb8 {
  float R[9], t[3], twc[3], kb8[8];
} orbx_frame_pose_kb8;
int orbx_project_map_points_fisheye_batch(orbx_extractor* ex, int n_frames, const orbx_frame_pose_kb8* left_poses,
                                          const orbx_frame_pose_kb8* right_poses, float min_x, float min_y, float max_x, float max_y,
                                          float viewing_cos_limit, const uint8_t* skip, orbx_map_point_view* views_out,
                                          orbx_map_point_right* views_right_out);


/* Replaces ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)
 * (src/ORBmatcher.cc:41-221) for F.Nleft != -1: left-camera search, right-camera search (radius not scaled by th, :144),
 * and the assignments to the stereo partner slots (:126-132, :199-204).  occupied / match have N entries, the right
 * keypoint i at n_left + i; semantics as orbx_search_by_projection.  Returns nmatches or an error. */
int orbx_search_by_projection_fisheye(int device, const orbx_keypoint* kps, const uint8_t* desc, int n_left, int n_right,
                                      float min_x, float min_y, float max_x, float max_y, const float* scale_factors,
                                      int nlevels, const orbx_map_point_view* map_points,
                                      const orbx_map_point_right* map_points_right, int n_map_points, float th,
                                      int far_points, float th_far_points, float nnratio, const int32_t* left_to_right,
                                      const int32_t* right_to_left, uint8_t* occupied, int32_t* match);

/* Replaces the matching part of ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
 * (src/ORBmatcher.cc:1594-1806) for CurrentFrame.Nleft != -1: uv_right = the caller's projection of every point into the
 * right camera (2 floats per point, :1705-1706); the right search runs only when the left one found candidates
 * (:1651).  Returns nmatches after the rotation-consistency cull. */
int orbx_search_by_projection_frame_fisheye(int device, const orbx_keypoint* kps, const uint8_t* desc, int n_left,
                                            int n_right, float min_x, float min_y, float max_x, float max_y,
                                            const orbx_projected_point* points, const float* uv_right, int n_points,
                                            int check_orientation, uint8_t* occupied, int32_t* match);
/* The two stereo-fisheye flavours above on the two-camera frames of an extraction BATCH: frame f = left image first_left + f and
 * right image first_right + f of `ex`'s last batch (keypoints / descriptors stay in HBM; scale factors = the handle's).  Points of
 * frame f are [f * points_stride .. + n_points[f]) of map_points / map_points_right (points / uv_right [.][2] for the frame
 * flavour); left_to_right / right_to_left are [n_frames][cap] (mvLeftToRightMatch / mvRightToLeftMatch of every frame, cap =
 * orbx_batch_results_device's cap); occupied_in (may be NULL = all free) / occupied / match are [n_frames][2 cap], row = [left
 * keypoints | right keypoints] like the one-shot calls' N = Nleft + Nright arrays; n_matches [n_frames].  Every kernel of the
 * chain runs ONCE for all frames and both cameras with a fixed number of fixed-point rounds enqueued blindly; a frame that needs
 * more (or larger candidate / writer lists) is redone through the one-shot path: results are those of n_frames separate calls.
 * map_points == NULL && map_points_right == NULL (round 6): the views of both cameras come from the handle's last
 * orbx_project_map_points_fisheye_batch (points_stride and every n_map_points[f] must equal the uploaded map's n).
 * Returns the total number of matches or a negative error. */
int orbx_search_by_projection_fisheye_batch(orbx_extractor* ex, int first_left, int first_right, int n_frames, float min_x, float min_y,
                                            float max_x, float max_y, const orbx_map_point_view* map_points,
                                            const orbx_map_point_right* map_points_right, const int32_t* n_map_points,
                                            int points_stride, float th, int far_points, float th_far_points, float nnratio,
                                            const int32_t* left_to_right, const int32_t* right_to_left, const uint8_t* occupied_in,
                                            uint8_t* occupied, int32_t* match, int32_t* n_matches);
int orbx_search_by_projection_frame_fisheye_batch(orbx_extractor* ex, int first_left, int first_right, int n_frames, float min_x,
                                                  float min_y, float max_x, float max_y, const orbx_projected_point* points,
                                                  const float* uv_right, const int32_t* n_points, int points_stride,
                                                  int check_orientation, const uint8_t* occupied_in, uint8_t* occupied,
                                                  int32_t* match, int32_t* n_matches);

/* ---- pose optimisation: Optimizer::PoseOptimization (src/Optimizer.cc:781-1107) -------------------------------------------------
 * The last stage of the tracking step (callers src/Tracking.cc:2687, 2844, 2898, 2902, 3620, 3635, 3650), for pinhole / rectified
 * frames (pFrame->mpCamera2 == NULL): one mono edge (Huber delta (float)sqrt(5.991)) per keypoint with a map point and
 * mvuRight < 0, one stereo edge (u, v, uR; delta (float)sqrt(7.815)) otherwise, information I * mvInvLevelSigma2[octave]; four
 * rounds of at most 10 g2o Levenberg iterations (tau 1e-5, 10 trials), each round restarting from the frame's pose, only the
 * edges classified as inliers by the previous round active, the robust kernel dropped after round 2 and the loop left after a
 * round when fewer than 10 edges exist; classification by float(chi2) > 5.991f / 7.815f, outlier edges re-evaluated at the
 * round's estimate, inlier edges keeping the error of the optimizer's last (possibly rejected) trial.  DESIGN.md lists every rule.
 * Tolerance parity: doubles where the reference computes in double (the stereo error's invz in float, as there); the reduction
 * order over the edges, the 6x6 LDLT (here without pivoting; a pivot <= 0 or not finite is a failed factorisation) and the
 * device's sin / cos / sqrt differ from Eigen / glibc in the last bits, so poses agree with a float64 restatement to 2e-6 rad and
 * 1e-5 relative translation (the tests' bound), and a classification may differ where chi2 lies within rounding of its threshold.  A point at exactly z = 0 under an evaluated
 * pose is outside the contract (the reference divides by it).  Results are run-to-run identical (fixed reduction tree), and a
 * frame of the batch entry gives the same bits as the one-shot entry on the same data.
 * Pose as Sophus stores Tcw (quaternion x y z w, translation; in/out: the optimised pose on return, normalised as
 * Sophus::SO3f does) plus the Pinhole parameters and mbf.  48 bytes. */
typedef struct orbx_pose_opt_frame {
  float q[4], t[3], fx, fy, cx, cy, bf;
} orbx_pose_opt_frame;
/* One frame from host arrays: kps_un = mvKeysUn (n), u_right = mvuRight (NULL: every edge mono), world_pos [n][3] =
 * mvpMapPoints[i]->GetWorldPos() where has_point[i] != 0, inv_level_sigma2 = mvInvLevelSigma2 (nlevels).  outlier[i] (in/out) =
 * mvbOutlier: entries with a point receive the classification, the others keep the caller's value.  Returns nGood =
 * nInitialCorrespondences - nBad (0 with the pose untouched for fewer than 3 edges), or a negative error.  Arguments are validated
 * before any device is touched (n <= 15000, octaves in [0, nlevels), finite world positions, pose and camera). */
int orbx_pose_optimization(int device, const orbx_keypoint* kps_un, const float* u_right, const float* world_pos,
                           const uint8_t* has_point, int n, const float* inv_level_sigma2, int nlevels,
                           orbx_pose_opt_frame* frame, uint8_t* outlier);
/* The same for n_frames frames in ONE kernel launch (one workgroup per frame): frame f = image first_image + f of ex's last batch,
 * keypoints taken as mvKeysUn (like the other batched entries), mvInvLevelSigma2 = the handle's; stereo_pair0 >= 0 reads mvuRight
 * from pair stereo_pair0 + f of the handle's stereo results (orbx_stereo_match_batch or orbx_rgbd_depth_batch), -1 = monocular.
 * world_pos [n_frames][cap][3], has_point / outlier [n_frames][cap] (cap = orbx_batch_results_device's; rows past a frame's
 * keypoint count are not read or written), frames / n_good [n_frames]; n_trials (may be NULL) [n_frames] receives the number of
 * Levenberg trials (linear solves) the frame ran.  Returns ORBX_OK or a negative error. */
int orbx_pose_optimization_batch(orbx_extractor* ex, int first_image, int n_frames, int stereo_pair0, const float* world_pos,
                                 const uint8_t* has_point, orbx_pose_opt_frame* frames, uint8_t* outlier, int32_t* n_good,
                                 int32_t* n_trials);

/* PoseOptimization for KannalaBrandt8 frames: monocular KB8 (mpCamera2 == NULL) and stereo-fisheye rigs (mpCamera2 != NULL,
 * Optimizer.cc:903-984).  Keypoint i < n_left gets an EdgeSE3ProjectXYZOnlyPose on the left camera, observation mvKeys[i] (for
 * monocular KB8 mvKeysUn, equal to mvKeys since Settings zeroes mDistCoef); i >= n_left an EdgeSE3ProjectXYZOnlyPoseToBody on the
 * right camera, observation mvKeysRight[i - n_left], mTrl = SE3Quat(Trl) (normalised).  Every edge: Huber delta (float)sqrt(5.991),
 * information I * mvInvLevelSigma2[octave], classification by float(chi2) > 5.991f; right edges count in nBad like left ones and
 * in the `edges < 10` rule; mvuRight is not read.  The rounds, Levenberg rules and classification are those of
 * orbx_pose_optimization.  KannalaBrandt8::project(Vector3d) narrows to float for theta = atan2f(sqrtf(x^2 + y^2), z) and
 * psi = atan2f(y, x) (here: sqrtf correctly rounded, atan2f = the double atan2 rounded once to float, within 1 ulp of glibc's);
 * the polynomial, cos / sin and projectJac run in double.  The to-body error maps Xw through (mTrl * T) (composed, then
 * normalised), its Jacobian through mTrl.map(T.map(Xw)) and mTrl's rotation matrix, as the reference does.  KB8 does not divide by
 * z: points behind a camera (theta > pi/2) keep finite errors and stay in the solve.  A point at exactly x = y = 0 in a camera
 * under an evaluated pose is outside the contract (projectJac divides by sqrt(x^2 + y^2)).  Tolerance parity as DESIGN.md states.
 * Frame: Tcw as Sophus stores it (q x y z w, t; in/out as orbx_pose_opt_frame), the eight KB8 parameters (fx fy cx cy k0..k3) of
 * the left and the right camera, and Trl = GetRelativePoseTrl() as Sophus stores it (q x y z w, t).  The right camera and Trl are
 * validated and used only when the frame has right keypoints.  120 bytes. */
typedef struct orbx_pose_opt_frame_kb8 {
  float q[4], t[3], kb8_left[8], kb8_right[8], trl_q[4], trl_t[3];
} orbx_pose_opt_frame_kb8;
/* One frame from host arrays: kps holds N = n_left + n_right keypoints, the left camera's raw keypoints then the right camera's
 * (n_right = 0: monocular KB8); world_pos [N][3], has_point / outlier [N] as orbx_pose_optimization.  Returns nGood or a negative
 * error; arguments are validated before any device is touched (N <= 15000, octaves in [0, nlevels), finite world positions,
 * pose, KB8 parameters and Trl, no zero quaternion). */
int orbx_pose_optimization_kb8(int device, const orbx_keypoint* kps, int n_left, int n_right, const float* world_pos,
                               const uint8_t* has_point, const float* inv_level_sigma2, int nlevels,
                               orbx_pose_opt_frame_kb8* frame, uint8_t* outlier);
/* The same for n_frames frames of ex's last extraction batch in ONE launch: frame f = left image first_left + f and right image
 * first_right + f (first_right = -1: monocular KB8), keypoints as extracted (the raw keypoints the fisheye matchers read).
 * world_pos [n_frames][2 cap][3], has_point / outlier [n_frames][2 cap]: the row layout of orbx_search_by_projection_fisheye_batch's
 * occupied / match (left keypoint i at i, right keypoint j at n_left(f) + j, cap = orbx_batch_results_device's), so the matcher's
 * match >= 0 is has_point as it stands; entries past a frame's n_left + n_right are not read or written.  frames / n_good /
 * n_trials (may be NULL) [n_frames].  A frame gives the bits of the one-shot entry on the same data.  Returns ORBX_OK or a
 * negative error. */
int orbx_pose_optimization_fisheye_batch(orbx_extractor* ex, int first_left, int first_right, int n_frames, const float* world_pos,
                                         const uint8_t* has_point, orbx_pose_opt_frame_kb8* frames, uint8_t* outlier,
                                         int32_t* n_good, int32_t* n_trials);


/* ---- two-view reconstruction (monocular initialisation) ----------------------------------------------- */

/* TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc:42-136; Tracking::MonocularInitialization, src/Tracking.cc:
 * 2451, through Pinhole::ReconstructWithTwoViews): `iterations` RANSAC hypotheses each for a homography and a fundamental
 * matrix from the same 8-point sets, scored on every match (CheckHomography / CheckFundamental), model selection by
 * RH = SH / (SH + SF), motion decomposition (ReconstructH: Faugeras' eight hypotheses; ReconstructF: DecomposeE's four) and
 * CheckRT (linear triangulation, cheirality, reprojection and parallax gates) -- all on the device, five launches for any
 * number of pairs.  Per-match arithmetic is float in the reference's expression order; the null vectors and the 3 x 3 SVDs are
 * solved in double (one-sided Jacobi) and narrowed, so results agree with the reference to rounding, not bit for bit
 * ("Two-view reconstruction").  Deterministic: fixed reduction trees, the same bits on every run, and pair f of
 * the batch entry gives the bits of the one-shot entry on the same data.
 *
 * Deliberate differences from the reference:
 *  - the 8-point index sets are an INPUT (`sets`, [iterations][8] indices into the match list = the (i, matches12[i]) with
 *    matches12[i] >= 0 in ascending i).  The reference draws them with rand() seeded once per process, so they are no function
 *    of the inputs; csrc/TwoViewReconstruction.h and the Python wrapper draw them the reference's way from the host's libc.
 *  - ReconstructH never assigns vP3D on success in the reference (:774-780; the caller reads a stale mvIniP3D); here the
 *    winning hypothesis' points are returned for both models and `model` reports which one won.
 *  - the RH threshold is the parameter rh_threshold (reference: 0.50; its comment names 0.40 - 0.45).
 *  - fewer than 8 matches (the reference indexes an empty vector): ok = 0 with n_matches set, p3d / triangulated zeroed,
 *    `sets` not read.  Whenever ok = 0, p3d and triangulated are zeroed (the reference leaves them untouched).
 *  - a set index outside [0, n_matches) or repeated within its set is ORBX_E_BADARG.
 *  - keypoints are undistorted pinhole keypoints (mvKeysUn) and K a pinhole matrix: KannalaBrandt8::ReconstructWithTwoViews
 *    (src/CameraModels/KannalaBrandt8.cpp:186-219) runs cv::fisheye::undistortPoints first, which stays with the caller. */
typedef struct orbx_two_view_params {
  float fx, fy, cx, cy;  /* mK */
  float sigma;           /* mSigma (1.0 in the reference) */
  float rh_threshold;    /* 0.50f in the reference */
  int32_t iterations;    /* mMaxIterations (200), in [1, 4096] */
} orbx_two_view_params;
typedef struct orbx_two_view_result { /* one per pair */
  int32_t ok;             /* Reconstruct's return value */
  int32_t model;          /* 0 = homography, 1 = fundamental (valid when score_h + score_f != 0) */
  int32_t best_h, best_f; /* winning hypothesis index per model, -1 when every score was 0 */
  float score_h, score_f; /* SH, SF */
  int32_t n_matches;      /* N */
  int32_t n_inliers;      /* inliers of the chosen model's winning hypothesis */
  int32_t n_good;         /* nGood of the chosen motion hypothesis */
  float parallax;         /* its parallax, degrees */
  float q[4], t[3];       /* T21 as Sophus stores it (x y z w, t), valid when ok */
} orbx_two_view_result;
/* One pair from host arrays.  kps1 / kps2: n1 / n2 undistorted keypoints, each count in [0, 15000]; matches12: n1 entries in
 * [-1, n2); sets: [iterations][8]; p3d ([n1][3], frame-1 camera coordinates) and triangulated ([n1]) are indexed by frame-1
 * keypoint like vP3D / vbTriangulated, entries of unmatched keypoints are 0; hyp_scores (may be NULL): [2][iterations], every
 * hypothesis' score, homography then fundamental.  All arguments are validated before a device is touched; valid arguments
 * without a device return ORBX_E_NODEVICE (there is no host path). */
int orbx_reconstruct_two_views(int device, const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2,
                               const int32_t* matches12, const int32_t* sets, const orbx_two_view_params* params,
                               orbx_two_view_result* result, float* p3d, uint8_t* triangulated, float* hyp_scores);
/* n_frames pairs in the layout orbx_search_for_initialization_batch produces: frame 2 of pair f = image first_image + f of the
 * handle's last batch (its keypoints, taken as mvKeysUn, stay on the device), frame 1 = kps1[f * stride ...) with n1[f]
 * keypoints, matches12 [n_frames][stride] as that call wrote it, sets [n_frames][iterations][8], results [n_frames],
 * p3d [n_frames][stride][3], triangulated [n_frames][stride], hyp_scores (may be NULL) [n_frames][2][iterations].  One upload,
 * one chain of five launches for all pairs, one download. */
int orbx_reconstruct_two_views_batch(orbx_extractor* ex, int first_image, int n_frames, const orbx_keypoint* kps1,
                                     const int32_t* n1, int stride, const int32_t* matches12, const int32_t* sets,
                                     const orbx_two_view_params* params, orbx_two_view_result* results, float* p3d,
                                     uint8_t* triangulated, float* hyp_scores);


/* ---- relocalisation PnP (MLPnPsolver RANSAC) ----------------------------------------------------------- */

/* MLPnPsolver (src/MLPnPsolver.cpp, include/MLPnPsolver.h; Tracking::Relocalization, src/Tracking.cc:3563-3594): the RANSAC of
 * `iterate` (:107-223) over minimal sets of six correspondences -- computePose (:354-666: planar test, design matrix, the
 * eigenvector of A^T A's smallest eigenvalue, the nearest rotation, scale, sign candidates, five Gauss-Newton steps),
 * CheckInliers (:265-295), Refine (:297-351) and the fall-back to the best hypothesis -- on the device, three launches for any
 * number of solvers: prepare (bearing vectors, null-space bases, mvMaxError), hypotheses (one wave per (solver, set): every set
 * the call could reach is solved and scored), replay (one workgroup per solver walks the hypotheses in order and takes the
 * decisions of the serial loop, running Refine where the loop would).  Solver arithmetic is double as in the reference;
 * CheckInliers keeps the reference's mixed rule (camera coordinates = double sums narrowed to float, then
 * GeometricCamera::project(cv::Point3f) in float, error2 < mvSigma2[i] * th2 in float).  The eigenvector and the 3 x 3 SVDs come
 * from one-sided Jacobi sweeps, the 6 x 6 solve from an unpivoted LDLT, sums from a fixed reduction tree: hypothesis poses agree
 * with a float64 restatement to rounding ("Relocalisation PnP"), not bit for bit.  Deterministic: the same bits on every
 * run, and problem p of the batch entry gives the bits of the one-shot entry on the same data.
 *
 * Deliberate differences from the reference:
 *  - the six-point index sets are an INPUT (`sets`, [n_sets][6] indices into the correspondence list = the keypoints i < n_left
 *    with has_point[i] != 0, in ascending i).  The reference draws them with rand(); csrc/MLPnPsolver.h and the Python wrapper
 *    draw them the reference's way from the host's libc.  Set j is the j-th pass of this call's loop; the call reads
 *    max(max_iterations - state.iterations, call_iterations) sets and n_sets must be at least that.  An index outside the list or
 *    repeated within its set is ORBX_E_BADARG; min_set other than 6 is ORBX_E_BADARG (the reference's `epsilon^3` and its
 *    six-point sign test assume it).
 *  - the solver's members that survive a call (mnIterations, mnBestInliers, mBestTcw, mvbBestInliers) are the in/out `state` and
 *    `best_mask`; a zeroed state is a fresh solver, the returned one continues it.  state.best_inliers must equal the number of
 *    correspondences flagged in best_mask (ORBX_E_BADARG otherwise).
 *  - the null-space basis of a bearing vector is a fixed one (JacobiSVD picks a basis; A^T A, J^T J and J^T r do not depend on it).
 *  - Eigen's pivoted LDLT is an unpivoted one; a pivot <= 0 or not finite leaves Gauss-Newton like the |dx| guard does.
 *  - orbx_mlpnp_ransac_parameters with no correspondence (the reference divides by N): max_iterations_out = 1.
 *  - the covariance branch of computePose is dead in the reference (covs(1)) and is not built.
 *  - KannalaBrandt8::unproject's std::tan(float) is taken as the double tangent rounded once to float (what a correctly rounded
 *    tanf returns; glibc's tanf is that from 2.41 on, within 1 ulp before), not the device's tanf: one float ulp in a bearing
 *    vector moves a six-point pose by 1e-7, orders above what the solver's arithmetic leaves open.
 * Out of contract: omega = 0 exactly inside Gauss-Newton (the reference's Jacobian divides by |omega|^2), a correspondence at
 * z = 0 (pinhole) under an evaluated pose. */
#define ORBX_CAMERA_PINHOLE 0
#define ORBX_CAMERA_KB8 1
typedef struct orbx_mlpnp_params {
  int32_t model;           /* ORBX_CAMERA_PINHOLE | ORBX_CAMERA_KB8 */
  float cam[8];            /* fx fy cx cy, then k0..k3 (KB8; not read for pinhole) */
  float kb8_precision;     /* KannalaBrandt8::precision of unproject's Newton loop (1e-6 in the reference; KB8 only) */
  float th2;               /* 5.991 at the call site */
  int32_t min_set;         /* 6 */
  int32_t min_inliers;     /* mRansacMinInliers as SetRansacParameters adjusted it (orbx_mlpnp_ransac_parameters), >= 6 */
  int32_t max_iterations;  /* mRansacMaxIts as adjusted, in [1, 4096] */
  int32_t call_iterations; /* iterate's nIterations (5 at the call site), in [0, 4096] */
} orbx_mlpnp_params;       /* 60 bytes */
typedef struct orbx_mlpnp_state {
  int32_t iterations;      /* mnIterations */
  int32_t best_inliers;    /* mnBestInliers */
  float best_Tcw[12];      /* top three rows of mBestTcw, row-major */
} orbx_mlpnp_state;        /* 56 bytes */
typedef struct orbx_mlpnp_result {
  int32_t ok;                /* iterate's return value */
  int32_t no_more;           /* bNoMore */
  int32_t n_inliers;         /* nInliers */
  int32_t n_correspondences; /* N */
  int32_t iterations_run;    /* passes of the loop in this call */
  int32_t hypothesis;        /* index of the set at which Refine succeeded and the call returned, -1 otherwise */
  int32_t refined;           /* 1 = Tcw is Refine's pose, 0 = the best hypothesis' own (fall-back, :209-220) or none */
  float Tcw[12];             /* top three rows of Tout, row-major (double pose narrowed to float); identity when ok == 0 */
} orbx_mlpnp_result;         /* 76 bytes */
/* SetRansacParameters (:225-263) in its own arithmetic: nMinInliers = int(N * epsilon) through float, raised to min_inliers and
 * min_set; epsilon raised to (float)minInliers / N; iterations = ceil(log(1 - p) / log(1 - pow(epsilon, 3))) (the cube is the
 * reference's, whatever min_set), 1 when minInliers == N; max(1, min(iterations, max_iterations)).  Pure host code.  Outputs may
 * be NULL.  Returns ORBX_OK, or ORBX_E_BADARG for a negative count. */
int orbx_mlpnp_ransac_parameters(int n_correspondences, double probability, int min_inliers, int max_iterations, int min_set,
                                 float epsilon, int32_t* min_inliers_out, int32_t* max_iterations_out, float* epsilon_out);
/* One solver, one `iterate` call, from host arrays: kps_un = mvKeysUn (n <= 15000; only the first n_left are read, n_left = n
 * unless the frame carries right-camera keypoints behind them), world_pos [n][3] / has_point [n] = vpMapPointMatches (non-NULL
 * and not bad), level_sigma2 = mvLevelSigma2 (nlevels).  best_mask [n] (in/out) = mvbBestInliers by keypoint, inliers [n] =
 * vbInliers, hyp_inliers (may be NULL) [n_sets] = mnInliersi of every pass the call ran, -1 for sets it did not reach.
 * N < min_inliers: no_more = 1, nothing else runs, `sets` is not read.  All arguments are validated before a device is touched
 * (finite inputs, octaves in [0, nlevels)); valid arguments without a device return ORBX_E_NODEVICE (there is no host solver). */
int orbx_mlpnp_iterate(int device, const orbx_keypoint* kps_un, int n, int n_left, const float* world_pos,
                       const uint8_t* has_point, const float* level_sigma2, int nlevels, const orbx_mlpnp_params* params,
                       const int32_t* sets, int n_sets, orbx_mlpnp_state* state, uint8_t* best_mask, orbx_mlpnp_result* result,
                       uint8_t* inliers, int32_t* hyp_inliers);
/* n_problems solvers in one call: problem p uses the keypoints of image image[p] of the handle's last extraction batch (taken as
 * mvKeysUn, resident on the device; several problems may name one image -- the candidate key frames of a relocalising frame),
 * mvLevelSigma2 = the handle's.  world_pos [n_problems][cap][3], has_point / best_masks / inliers [n_problems][cap] (cap =
 * orbx_batch_results_device's; the row layout orbx_search_by_bow_batch writes `matches` in, has_point = matches >= 0; entries
 * past an image's keypoint count are not read or written), params / states / results [n_problems], sets [n_problems][n_sets][6],
 * hyp_inliers (may be NULL) [n_problems][n_sets].  One upload, three launches, one download.  At most 65535 problems.
 * Pointers, counts, image indices, params and states are validated before a device is touched; world_pos, best_masks and the sets
 * depend on the images' keypoint counts, which live on the device, and are validated after those are read, before any launch. */
int orbx_mlpnp_iterate_batch(orbx_extractor* ex, int n_problems, const int32_t* image, const float* world_pos,
                             const uint8_t* has_point, const orbx_mlpnp_params* params, const int32_t* sets, int n_sets,
                             orbx_mlpnp_state* states, uint8_t* best_masks, orbx_mlpnp_result* results, uint8_t* inliers,
                             int32_t* hyp_inliers);

/* ---- loop-closing Sim3 (Sim3Solver RANSAC) -------------------------------------------------------------- */

/* Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h; LoopClosing::DetectCommonRegionsFromBoW, src/LoopClosing.cc:761-779): the
 * RANSAC of `iterate` (:147-281) over triples of correspondences -- ComputeSim3 (:296-396: Horn's closed form) and CheckInliers
 * (:398-418: both reprojections against the integer thresholds, no depth test) -- on the device, three launches for any number of
 * solvers: prepare (the constructor, :34-118: the ordered correspondence list, X3Dc1 = Rcw1 Xw1 + tcw1 and X3Dc2 in float, their
 * projections, mvnMaxError = 9.210 * mvLevelSigma2[octave] TRUNCATED to an integer as the reference's vector<size_t> does),
 * hypotheses (one wave per (solver, triple): every triple the call could reach is solved and scored), replay (one workgroup per
 * solver takes the decisions of the serial loop: `>=` replaces the best, so a later tie wins; `> min_inliers` converges).
 * CheckInliers is float arithmetic in the reference's expression order.  Deterministic: the same bits on every run, and problem
 * p of the batch entry gives the bits of the one-shot entry on the same data.
 *
 * The call site passes a non-empty vpKeyFrameMatchedMP, so pKFm is pKF2 for every correspondence; the caller resolves each map
 * point's index in its key frame and hands over the octave of that key point.  matched[i1] != 0 <=> vpMatched12[i1] is set, key
 * frame 1 has a map point at i1, neither point is bad and both indices are >= 0.
 *
 * Deliberate differences from the reference:
 *  - the triples are an INPUT (`sets`, [n_sets][3] indices into the correspondence list = the i1 with matched[i1] != 0, ascending).
 *    The reference draws them with rand(); csrc/Sim3Solver.h and the Python wrapper draw them the reference's way from the
 *    host's libc.  Set j is the j-th pass of this call's loop; the call reads min(max_iterations - state.iterations,
 *    call_iterations) sets and n_sets must be at least that.  An index outside the list or repeated within its set is
 *    ORBX_E_BADARG.
 *  - Horn's solve (centroids, M, the 4 x 4 N, its eigenvector by cyclic Jacobi rotations, the rotation, scale and translation) is
 *    double arithmetic on the float points; R, t and s are then narrowed to float, and T12 = [s R | t], T21 = [(1 / s) R^T |
 *    -(1 / s) R^T t] are formed in float from the narrowed values.  The reference solves in float with EigenSolver<Matrix4f>,
 *    which moves a squared reprojection error by up to 3.5e-3 of itself; the double solve leaves 5.9e-5 of a threshold.
 *  - the solver's members that survive a call (mnIterations, mnBestInliers, mBestRotation / Translation / Scale, mvbBestInliers)
 *    are the in/out `state` and `best_mask`; a zeroed state is a fresh solver.  state.best_inliers must equal the number of
 *    correspondences flagged in best_mask (ORBX_E_BADARG otherwise).
 *  - a call that does not converge returns the best hypothesis the STATE knows (R12, t12, s12, T12), also when no hypothesis of
 *    this call reached the carried best_inliers -- the bConverge overload of the reference returns an uninitialised matrix there,
 *    the other overload the identity.  A solver that has never run a pass returns the identity.
 *  - the first-wins merge of the covisibles' SearchByBoW lists (src/LoopClosing.cc:736-749) needs map-point identity and stays
 *    with the caller.
 * Out of contract: a triple whose two point sets are bitwise identical (|v| == 0 exactly: 0 / 0 in the reference too); the call
 * returns, with results unspecified. */
typedef struct orbx_sim3_params {
  int32_t model1;          /* camera of key frame 1: ORBX_CAMERA_PINHOLE | ORBX_CAMERA_KB8 */
  float cam1[8];           /* fx fy cx cy, then k0..k3 (KB8; not read for pinhole) */
  int32_t model2;          /* camera of key frame 2 */
  float cam2[8];
  float kb8_precision;     /* KannalaBrandt8::precision (validated for KB8 cameras; project does not read it) */
  int32_t fix_scale;       /* mbFixScale: s = 1 */
  int32_t min_inliers;     /* mRansacMinInliers (15 at the call site), >= 3 */
  int32_t max_iterations;  /* mRansacMaxIts as SetRansacParameters adjusted it (orbx_sim3_ransac_parameters), in [1, 4096] */
  int32_t call_iterations; /* iterate's nIterations (20 at the call site), in [0, 4096] */
} orbx_sim3_params;        /* 92 bytes */
typedef struct orbx_sim3_state {
  int32_t iterations;      /* mnIterations */
  int32_t best_inliers;    /* mnBestInliers */
  float best_R[9];         /* mBestRotation, row-major */
  float best_t[3];         /* mBestTranslation */
  float best_s;            /* mBestScale */
} orbx_sim3_state;         /* 60 bytes */
typedef struct orbx_sim3_result {
  int32_t converged;         /* bConverge: a hypothesis with more than min_inliers inliers that also took the best */
  int32_t no_more;           /* bNoMore */
  int32_t n_inliers;         /* nInliers (0 unless converged) */
  int32_t n_correspondences; /* N */
  int32_t iterations_run;    /* passes of the loop in this call */
  int32_t hypothesis;        /* index (within this call's sets) of the set that converged, -1 otherwise */
  float R12[9], t12[3], s12; /* the converged hypothesis, else the best one the state knows (identity before any pass) */
  float T12[12];             /* top three rows of [s12 R12 | t12], row-major */
} orbx_sim3_result;          /* 124 bytes */
/* SetRansacParameters (:120-145) in its own arithmetic: epsilon = (float)min_inliers / N, iterations = ceil(log(1 - p) /
 * log(1 - pow(epsilon, 3))), 1 when min_inliers == N; max(1, min(iterations, max_iterations)).  No correspondence (the reference
 * divides by N): 1.  Pure host code.  Returns ORBX_OK, or ORBX_E_BADARG for a negative count. */
int orbx_sim3_ransac_parameters(int n_correspondences, double probability, int min_inliers, int max_iterations,
                                int32_t* max_iterations_out);
/* One solver, one `iterate` call, from host arrays over the n = vpMatched12.size() key points of key frame 1 (n <= 15000):
 * Tcw1 / Tcw2 = the key frames' poses (top three rows, row-major), world_pos1 [n][3] = the world position of key frame 1's map
 * point at i1, world_pos2 [n][3] = that of vpMatched12[i1], matched [n] (above), octave1 / octave2 [n] = the octaves of the two
 * points' key points in their key frames, level_sigma2_1 / _2 = the key frames' mvLevelSigma2.  Entries with matched == 0 are not
 * read.  best_mask [n] (in/out) = mvbBestInliers by i1, inliers [n] = vbInliers (zero unless converged), hyp_inliers (may be
 * NULL) [n_sets] = mnInliersi of every pass the call ran, -1 for sets it did not reach.  N < min_inliers: no_more = 1, nothing
 * else runs, `sets` is not read.  All arguments are validated before a device is touched (finite poses, positions, cameras and
 * state; level_sigma2 in [0, 1e9]; octaves in [0, nlevels)); valid arguments without a device return ORBX_E_NODEVICE (there is
 * no host solver). */
int orbx_sim3_iterate(int device, int n, const float* Tcw1, const float* Tcw2, const float* world_pos1, const float* world_pos2,
                      const uint8_t* matched, const int32_t* octave1, const int32_t* octave2, const float* level_sigma2_1,
                      int nlevels1, const float* level_sigma2_2, int nlevels2, const orbx_sim3_params* params, const int32_t* sets,
                      int n_sets, orbx_sim3_state* state, uint8_t* best_mask, orbx_sim3_result* result, uint8_t* inliers,
                      int32_t* hyp_inliers);
/* n_problems solvers in one call (the candidates of a key frame, loop and merge class): n [n_problems] key points per problem
 * (<= cap <= 15000), Tcw1 / Tcw2 [n_problems][12], world_pos1 / world_pos2 [n_problems][cap][3], matched / octave1 / octave2 /
 * best_masks / inliers [n_problems][cap] (entries past n[p] are not read or written), the two level_sigma2 tables shared by all
 * problems, params / states / results [n_problems], sets [n_problems][n_sets][3], hyp_inliers (may be NULL)
 * [n_problems][n_sets].  One upload, three launches, one download.  At most 65535 problems.  Validated like the one-shot entry. */
int orbx_sim3_iterate_batch(int device, int n_problems, int cap, const int32_t* n, const float* Tcw1, const float* Tcw2,
                            const float* world_pos1, const float* world_pos2, const uint8_t* matched, const int32_t* octave1,
                            const int32_t* octave2, const float* level_sigma2_1, int nlevels1, const float* level_sigma2_2,
                            int nlevels2, const orbx_sim3_params* params, const int32_t* sets, int n_sets, orbx_sim3_state* states,
                            uint8_t* best_masks, orbx_sim3_result* results, uint8_t* inliers, int32_t* hyp_inliers);

/* ---- loop-closing Sim3 refinement (Optimizer::OptimizeSim3) --------------------------------------------- */

/* Optimizer::OptimizeSim3 (src/Optimizer.cc:2164-2424; the call sites src/LoopClosing.cc:609, 852), the step between the Sim3
 * searches of loop closing and map merging, on the device: ONE launch, one wave per problem, for any number of problems.
 *
 * Edges, per key point i of key frame 1 with matched[i] != 0 (<=> vpMatches1[i] is set, key frame 1 has a map point at i and
 * neither point is bad; the entries the reference skips without clearing or counting are the caller's): P3D1c = R1w Xw1 + t1w and
 * P3D2c = R2w Xw2 + t2w in float (the expression of the Sim3 solver's X3Dc), widened to double.  Skipped: idx2[i] < 0 with
 * all_points == 0, and P3D2c.z < 0 (strict: z == 0 passes).  Otherwise nCorrespondences++ and two edges: e12 = obs1 - pi1(S12
 * P3D2c), obs1 = kps1_un[i], information mvInvLevelSigma2_1[octave]; e21 = obs2 - pi2(S12^-1 P3D1c), information
 * mvInvLevelSigma2_2[octave2].  idx2 >= 0: obs2 and octave2 are kps2_un[idx2]'s.  idx2 < 0: obs2 = (x invz, y invz) of P3D2c
 * with a float invz = 1 / z -- NORMALISED coordinates, not pixels -- and octave2 = track_level2[i]: the reference's behaviour
 * with bAllPoints = true (both call sites), reproduced and not repaired; such a pair weighs on the first round under the Huber
 * kernel and is then almost always cleared.  Both edges carry a Huber kernel of delta = (float)sqrt(th2).
 *
 * Sim3 arithmetic (Thirdparty/g2o/g2o/types/sim3.h): oplus = Sim3(update) * estimate, update = (omega, upsilon, sigma),
 * update[6] = 0 with a fixed scale; Sim3(Vector7d) in its four branches (|sigma| < 1e-5, theta < 1e-5); r = Quaterniond(R) is NOT
 * normalised (unlike SE3Quat), nor do operator* and inverse() normalise; map(x) = s (r * x) + t with Eigen's quaternion-vector
 * formula; inverse() = (conj r, conj r * ((-1 / s) t), 1 / s).
 *
 * Levenberg (optimization_algorithm_levenberg.cpp:61-170), the rules of the pose optimiser in 7 dimensions: lambda = 1e-5 max
 * diag(H); a trial solves (H + lambda I) x = b by an unpivoted LDLT, a failed factorisation gives chi2 = DBL_MAX; rho = (chi -
 * trial chi) / (x . (lambda x + b) + 1e-3); accepted: lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)), ni = 2; rejected: lambda
 * *= ni, ni *= 2; at most 10 trials per iteration; an iteration that gains less than 1e-3 of its chi2 three times in a row
 * stops.  With a fixed scale row and column 6 of H hold only lambda.
 *
 * Rounds: optimize(5); every pair with e12.chi2() > th2 || e21.chi2() > th2 (in double, at the errors of the optimiser's LAST
 * TRIAL, even a rejected one) is removed and its matched entry cleared (n_bad); the survivors lose their robust kernel;
 * n_correspondences - n_bad < 10 returns 0 (early_return: matches already cleared, S12 untouched).  Then optimize(n_bad > 0 ?
 * 10 : 5) from round one's estimate; the errors are recomputed at the final estimate, entries above th2 are cleared, the others
 * counted (n_in); S12 becomes the estimate.  mAcumHessian is set to zero by the reference (after the early return's exit) and never
 * accumulated: the mirrors return zeros, and leave it alone on the early return.
 *
 * Deliberate differences from the reference:
 *  - the Jacobians are ANALYTIC.  Both edge classes leave linearizeOplus commented out, so g2o differentiates numerically
 *    (central differences, delta = 1e-9, base_binary_edge.hpp:130-205), which carries rounding noise of about eps |pi| / 1e-9 per
 *    entry that no implementation can reproduce bit for bit.  With y = S12 P3D2c, z = S12^-1 P3D1c, under the left perturbation:
 *    J12 = -Jpi1(y) [ -[y]x | I | y ], J21 = -Jpi2(z) (1 / s) R^T [ [P3D1c]x | -I | -P3D1c ]; column 6 is zero with a fixed scale.
 *    tests/sim3opt_cases.py checks them against central differences and measures what the difference does to the result.
 *  - PINHOLE cameras only: a KannalaBrandt8 model is ORBX_E_BADARG.  KannalaBrandt8::project(Vector3d) takes theta and psi
 *    through atan2f and sqrtf (KannalaBrandt8.cpp:48-66); a 1e-9 step does not move a float, so g2o's numeric Jacobian of a
 *    fisheye edge is zero or a one-ulp spike times 5e8: there is no behaviour to be faithful to.
 * Out of contract: a point at exactly z = 0 under an evaluated estimate (as in the pose optimiser). */
typedef struct orbx_sim3opt_params {
  int32_t model1;      /* camera of key frame 1: ORBX_CAMERA_PINHOLE (ORBX_CAMERA_KB8 is rejected, above) */
  float cam1[4];       /* fx fy cx cy */
  int32_t model2;      /* camera of key frame 2 */
  float cam2[4];
  float th2;           /* > 0 */
  int32_t fix_scale;   /* bFixScale */
  int32_t all_points;  /* bAllPoints */
} orbx_sim3opt_params; /* 52 bytes */
typedef struct orbx_sim3_pose {   /* g2o::Sim3 */
  double q[4];         /* r, x y z w, not normalised */
  double t[3];
  double s;            /* > 0 */
} orbx_sim3_pose;      /* 64 bytes */
typedef struct orbx_sim3opt_result {
  int32_t n_in;              /* the return value: nIn, 0 on the early return */
  int32_t n_correspondences; /* nCorrespondences = edge pairs */
  int32_t n_bad;             /* nBad of round one */
  int32_t n_in_kf2;          /* nInKF2 */
  int32_t n_out_kf2;         /* nOutKF2 */
  int32_t trials;            /* Levenberg trials of both rounds */
  int32_t early_return;      /* n_correspondences - n_bad < 10 */
} orbx_sim3opt_result;       /* 28 bytes */
/* One pair of key frames, from host arrays over the n = vpMatches1.size() key points of key frame 1 (n <= 15000): kps1_un [n] =
 * mvKeysUn of key frame 1, world_pos1 / world_pos2 [n][3] = the world positions of key frame 1's map point at i and of
 * vpMatches1[i], matched [n] (in/out, above: cleared entries become 0, the others keep their value), idx2 [n] = the index of
 * vpMatches1[i] in key frame 2 (< 0: not observed there), kps2_un [n2] = mvKeysUn of key frame 2, track_level2 [n] =
 * mnTrackScaleLevel of vpMatches1[i] (read, and checked, only where idx2 < 0 and all_points is set), Tcw1 / Tcw2 = the key frames'
 * poses (top three rows, row-major),
 * inv_level_sigma2_1 / _2 = their mvInvLevelSigma2.  Entries with matched == 0 are not read.  S12 is in/out and unchanged on the
 * early return.  Returns n_in (>= 0).  All arguments are validated before a device is touched (null pointers, sizes, finite
 * poses, positions, key points, cameras and tables, S12.s > 0 and a non-zero quaternion, th2 > 0, octaves and track_level2
 * inside their tables, idx2 < n2, pinhole models); valid arguments without a device return ORBX_E_NODEVICE (there is no host
 * optimiser). */
int orbx_optimize_sim3(int device, int n, const orbx_keypoint* kps1_un, const float* world_pos1, const float* world_pos2,
                       uint8_t* matched, const int32_t* idx2, const orbx_keypoint* kps2_un, int n2, const int32_t* track_level2,
                       const float* Tcw1, const float* Tcw2, const float* inv_level_sigma2_1, int nlevels1,
                       const float* inv_level_sigma2_2, int nlevels2, const orbx_sim3opt_params* params, orbx_sim3_pose* S12,
                       orbx_sim3opt_result* result);
/* n_problems pairs in one call (the candidates of a key frame: what the batched RANSAC in front of it hands over), laid out as
 * orbx_sim3_iterate_batch lays them out: n [n_problems] key points per problem (<= cap <= 15000, 0 is allowed), kps1_un / matched
 * / idx2 / track_level2 [n_problems][cap], world_pos1 / world_pos2 [n_problems][cap][3], kps2_un [n_problems][cap2] with n2
 * [n_problems] <= cap2 key points each, Tcw1 / Tcw2 [n_problems][12], the two mvInvLevelSigma2 tables shared by all problems,
 * params / S12 / results [n_problems].  Entries past n[p] are neither read nor written.  One upload, one launch, one download;
 * problem p has the bits of the one-shot entry on the same data.  At most 65535 problems.  Validated like the one-shot entry.
 * Returns ORBX_OK. */
int orbx_optimize_sim3_batch(int device, int n_problems, int cap, const int32_t* n, const orbx_keypoint* kps1_un,
                             const float* world_pos1, const float* world_pos2, uint8_t* matched, const int32_t* idx2,
                             const orbx_keypoint* kps2_un, int cap2, const int32_t* n2, const int32_t* track_level2,
                             const float* Tcw1, const float* Tcw2, const float* inv_level_sigma2_1, int nlevels1,
                             const float* inv_level_sigma2_2, int nlevels2, const orbx_sim3opt_params* params,
                             orbx_sim3_pose* S12, orbx_sim3opt_result* results);

/* ---- inertial pose optimisation (Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame) ------------- */

/* What Tracking::TrackLocalMap calls instead of PoseOptimization once the IMU is initialised (src/Tracking.cc:2896-2919):
 * Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:4544-4931) and PoseInertialOptimizationLastFrame
 * (:4933-5356), one workgroup per frame, the whole call in one launch (csrc/orbx_pose_inertial.hip): the frame's body pose,
 * velocity and biases under its reprojection edges (EdgeMonoOnlyPose where u_right < 0, EdgeStereoOnlyPose otherwise), the
 * inertial edge to the last key frame (fixed) or the previous frame (free, under its prior), the two bias random-walk edges,
 * four rounds of ten Gauss-Newton iterations with the classification after each, the recovery pass, and the new prior:
 * the Hessian at the final estimate, marginalised over the previous frame (last frame) and clamped to positive semi-definite.
 * DESIGN.md lists every rule.  Scope and deliberate differences:
 *  - pinhole / rectified frames with one camera (mpCamera2 == NULL, Nleft == -1); Pinhole::uncertainty2 is 1.  A frame with
 *    camera_model == ORBX_CAMERA_KB8 or n_cameras != 1 is ORBX_E_BADARG.
 *  - IMU preintegration stays with the caller: orbx_imu_preintegrated holds the fields of IMU::Preintegrated the edges read.
 *  - the dense 15 x 15 / 30 x 30 system is solved by an unpivoted LDLT where g2o's LinearSolverDense uses Eigen's pivoted one:
 *    the results differ by rounding.  A pivot <= 0 or not finite ends the round without applying an update and sets
 *    ORBX_PI_SOLVE_FAILED in status (g2o would apply the stale x of the iteration before and stop the round).
 *  - the inverse of C's 9 x 9 block is an unpivoted Gauss-Jordan (Eigen: partially pivoted LU); a block that is not positive
 *    definite sets ORBX_PI_BAD_COVARIANCE and returns the input state, n_good 0 and H zero.
 *  - Marginalize's pseudo-inverse comes from a symmetric eigen-decomposition (JacobiSVD in the reference): the block is
 *    symmetric positive semi-definite, its singular values are its eigenvalues; eigenvalues <= 1e-6 are dropped alike.
 *  - IMU::NormalizeRotation of GetDeltaRotation runs its SVD in double and rounds to float (a float JacobiSVD in the reference).
 * Two calls on the same input agree bit for bit (fixed reduction trees, no atomics). */
typedef struct orbx_imu_preintegrated {   /* IMU::Preintegrated, row-major floats as it stores them */
  float dR[9], dV[3], dP[3];
  float JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
  float C[225];          /* 15 x 15 covariance: rotation, velocity, position (9), gyro walk (3), accelerometer walk (3) */
  float b[6];            /* the linearisation bias: bax bay baz bwx bwy bwz */
  float dT;
} orbx_imu_preintegrated;
typedef struct orbx_imu_state {
  double Rwb[9], twb[3], vwb[3], bg[3], ba[3];
} orbx_imu_state;
typedef struct orbx_imu_prior {           /* ConstraintPoseImu (include/G2oTypes.h:671-707) */
  orbx_imu_state state;
  double H[225];
} orbx_imu_prior;
typedef struct orbx_pose_inertial_frame { /* what ImuCamPose(Frame*) and the bias / velocity vertices read (src/G2oTypes.cc:74-118) */
  float Rwb[9], twb[3], vwb[3];           /* GetImuRotation / GetImuPosition / GetVelocity */
  float bias[6];                          /* mImuBias: bax bay baz bwx bwy bwz */
  float Rcw[9], tcw[3];                   /* GetPose(): separate inputs, re-derived from the body pose only by the first update */
  float Rcb[9], tcb[3], tbc[3];           /* mImuCalib.mTcb, mImuCalib.mTbc.translation() */
  float fx, fy, cx, cy, bf;
  int32_t camera_model;                   /* ORBX_CAMERA_PINHOLE (0); ORBX_CAMERA_KB8 is rejected */
  int32_t n_cameras;                      /* 1; a second camera is rejected */
} orbx_pose_inertial_frame;
#define ORBX_PI_SOLVE_FAILED 1
#define ORBX_PI_BAD_COVARIANCE 2
typedef struct orbx_pose_inertial_result {
  orbx_imu_state state;                   /* the optimised Rwb, twb, velocity and biases (the frame takes their float casts) */
  double H[225];                          /* the new prior's Hessian (with `state`: the frame's ConstraintPoseImu) */
  int32_t n_good;                         /* nInitialCorrespondences - nBad: the reference's return value */
  int32_t n_inliers_mono, n_outliers_mono, n_inliers_stereo, n_outliers_stereo;   /* of the last classification */
  int32_t rounds;                         /* rounds run (1 when fewer than 10 edges, else 4) */
  int32_t status;                         /* 0, or ORBX_PI_* flags */
  int32_t recovered;                      /* 1 when the recovery pass (nInliers < 30 && !bRecInit) ran */
} orbx_pose_inertial_result;
/* kps_un / u_right (NULL: every edge mono) / world_pos [n][3] / has_point / track_depth (MapPoint::mTrackDepth) by key point,
 * n <= 15000; inv_level_sigma2 [nlevels].  outlier [n] receives mvbOutlier where has_point is set and keeps the caller's value
 * elsewhere.  A frame with no point at all is valid (the inertial edges alone).  Validated before any device is touched: counts,
 * octaves in [0, nlevels), everything finite, dT > 0, positive diagonals of C's 9 x 9 and two 3 x 3 blocks, a pinhole frame with
 * one camera, and (last frame) a prior H symmetric to rounding.  Returns n_good >= 0 or a negative error; valid arguments
 * without a device return ORBX_E_NODEVICE (there is no host path). */
int orbx_pose_inertial_optimization_last_keyframe(int device, const orbx_keypoint* kps_un, const float* u_right,
                                                  const float* world_pos, const uint8_t* has_point, const float* track_depth, int n,
                                                  const float* inv_level_sigma2, int nlevels, const orbx_pose_inertial_frame* frame,
                                                  const orbx_imu_state* keyframe_state, const orbx_imu_preintegrated* preintegrated,
                                                  int rec_init, uint8_t* outlier, orbx_pose_inertial_result* result);
/* prev_state: the previous frame's estimate; prior: its ConstraintPoseImu (the caller deletes it afterwards, :5352-5353);
 * preintegrated: mpImuPreintegrated (from the last key frame: the walk edges' information); preintegrated_frame:
 * mpImuPreintegratedFrame (from the previous frame: the inertial edge). */
int orbx_pose_inertial_optimization_last_frame(int device, const orbx_keypoint* kps_un, const float* u_right, const float* world_pos,
                                               const uint8_t* has_point, const float* track_depth, int n,
                                               const float* inv_level_sigma2, int nlevels, const orbx_pose_inertial_frame* frame,
                                               const orbx_imu_state* prev_state, const orbx_imu_prior* prior,
                                               const orbx_imu_preintegrated* preintegrated,
                                               const orbx_imu_preintegrated* preintegrated_frame, int rec_init, uint8_t* outlier,
                                               orbx_pose_inertial_result* result);
/* n_problems frames in one launch, laid out as orbx_optimize_sim3_batch lays them out: n [n_problems] key points per problem
 * (<= cap <= 15000, 0 is allowed), kps_un / u_right (may be NULL) / has_point / track_depth / outlier [n_problems][cap],
 * world_pos [n_problems][cap][3], one table of inv_level_sigma2, frames / states / priors / records / rec_init / results
 * [n_problems].  Entries past n[p] are neither read nor written.  Problem p has the bits of the one-shot entry on the same data.
 * At most 65535 problems.  Validated like the one-shot entries.  Returns ORBX_OK. */
int orbx_pose_inertial_optimization_last_keyframe_batch(int device, int n_problems, int cap, const int32_t* n,
                                                        const orbx_keypoint* kps_un, const float* u_right, const float* world_pos,
                                                        const uint8_t* has_point, const float* track_depth,
                                                        const float* inv_level_sigma2, int nlevels,
                                                        const orbx_pose_inertial_frame* frames, const orbx_imu_state* keyframe_states,
                                                        const orbx_imu_preintegrated* preintegrated, const int32_t* rec_init,
                                                        uint8_t* outlier, orbx_pose_inertial_result* results);
int orbx_pose_inertial_optimization_last_frame_batch(int device, int n_problems, int cap, const int32_t* n,
                                                     const orbx_keypoint* kps_un, const float* u_right, const float* world_pos,
                                                     const uint8_t* has_point, const float* track_depth,
                                                     const float* inv_level_sigma2, int nlevels,
                                                     const orbx_pose_inertial_frame* frames, const orbx_imu_state* prev_states,
                                                     const orbx_imu_prior* priors, const orbx_imu_preintegrated* preintegrated,
                                                     const orbx_imu_preintegrated* preintegrated_frame, const int32_t* rec_init,
                                                     uint8_t* outlier, orbx_pose_inertial_result* results);
/* Test hook: the dense pieces and SO(3) functions the inertial solvers add to csrc/orbx_linalg.h, each alone on n items of
 * doubles (orbx_debug_linalg keeps its own operations and numbers).  One wave per item for the dense pieces, in the call
 * sites' register layout; one thread per item for SO(3).  out is read as well as written.
 *   op                          in, per item                        out, per item
 *   ORBX_ILA_LDLT15 / _LDLT30   H [N][N] (lower triangle read), b [N]   x [N] (the caller's values when it fails), flag
 *   ORBX_ILA_EIG9 / _EIG15      A [N][N] symmetric                  w [N], V [N][N] (row-major, column j pairs with w[j])
 *   ORBX_ILA_CLAMP15            A [15][15]                          the clamped matrix [15][15]
 *   ORBX_ILA_PINV15             A [15][15]                          the pseudo-inverse [15][15] (eigenvalues <= 1e-6 dropped)
 *   ORBX_ILA_INVERSE9           A [9][9] positive definite          the inverse [9][9] (the caller's values when it fails), flag
 *   ORBX_ILA_EXP_SO3            w [3]                               R [3][3]
 *   ORBX_ILA_LOG_SO3            R [3][3]                            w [3]
 *   ORBX_ILA_JR / _JR_INV       v [3]                               RightJacobianSO3 / InverseRightJacobianSO3 [3][3]
 *   ORBX_ILA_NORMALIZE_F        R [3][3] (floats widened)           IMU::NormalizeRotation, floats widened [3][3]
 * A null pointer, n outside [1, ORBX_ILA_MAX_ITEMS] and an unknown op are ORBX_E_BADARG before any device is touched. */
#define ORBX_ILA_LDLT15 0
#define ORBX_ILA_LDLT30 1
#define ORBX_ILA_EIG9 2
#define ORBX_ILA_EIG15 3
#define ORBX_ILA_CLAMP15 4
#define ORBX_ILA_PINV15 5
#define ORBX_ILA_INVERSE9 6
#define ORBX_ILA_EXP_SO3 7
#define ORBX_ILA_LOG_SO3 8
#define ORBX_ILA_JR 9
#define ORBX_ILA_JR_INV 10
#define ORBX_ILA_NORMALIZE_F 11
#define ORBX_ILA_OPS 12
#define ORBX_ILA_MAX_ITEMS 4096
int orbx_debug_inertial_linalg(int device, int op, int n, const void* in, void* out);

/* ---- local bundle adjustment (Optimizer::LocalBundleAdjustment) ------------------------------------------ */

/* The visual Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*, int&, int&, int&, int&) (src/Optimizer.cc:1109-1516; the
 * call site src/LocalMapping.cc, after CreateNewMapPoints and SearchInNeighbors), one problem per call, on the device: g2o's
 * Levenberg on BlockSolver_6_3 -- pose vertices of 6, marginalised point vertices of 3 -- restated as a chain of kernels
 * (csrc/orbx_lba.hip), all arithmetic in double.
 *
 * The problem is a flat graph.  Key frames: the n_local key frames of lLocalKeyFrames first (the current key frame, then its
 * covisibles), then the n_fixed of lFixedCameras; a local key frame with fixed != 0 is the map's initial key frame (a fixed
 * vertex); every key frame of the second group must carry fixed != 0.  Poses are Tcw as Sophus stores it (float unit quaternion
 * x y z w, float translation), widened and normalised as SE3Quat(q, t) does.  Points: lLocalMapPoints in list order, float.
 * Edges: in the reference's order -- points in list order (edge.point never decreases), each point's observations in the
 * caller's order -- one per (key frame, point) at most, as a point's observations are a map.  u_right < 0: EdgeSE3ProjectXYZ
 * (src/OptimizableTypes.cpp:136-157; error obs - Pinhole::project, float parameters times double, chi2 gate 5.991, Huber delta
 * (float)sqrt(5.991)); u_right >= 0: g2o::EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.cpp:190-274; a FLOAT invz = 1.0f / z in
 * the error, the Jacobian in double, gate 7.815, delta (float)sqrt(7.815)).  The information value is inv_sigma2 widened.
 *
 * Levenberg (optimization_algorithm_levenberg.cpp:61-184) with the Schur complement of block_solver.hpp:354-447: lambda starts
 * at 1e-5 times the largest |H_jj| over the pose and point diagonals, or at lambda_init when that is positive (100 for inertial
 * maps, Optimizer.cc:1200); a trial adds lambda to both diagonals, forms Dinv = (Hll + lambda I)^-1, Hschur = Hpp + lambda I -
 * sum Hpl Dinv Hpl^T, bschur = bp - sum Hpl Dinv bl, factors the dense 6 n system by an unpivoted LDLT (a pivot <= 0 or not
 * finite fails the solve: x keeps its value and the trial's chi2 is DBL_MAX), back-substitutes xl = Dinv (bl - Hpl^T xp) and
 * applies SE3Quat::exp(xp) * pose and point + xl to a trial copy; rho = (chi - trial chi) / (sum over ALL of x of x (lambda x + b)
 * + 1e-3); accept, reject, the lambda update, at most 10 trials per iteration, rho == 0 and the three-small-gains stop as in the
 * pose optimiser.  Afterwards an edge is flagged for erasure when its chi2 -- the one it holds after the optimiser's LAST TRIAL,
 * even a rejected one -- exceeds its gate, or when its depth at the FINAL estimates is not positive.
 *
 * A key frame without an edge, and a point without one, take no part (g2o's active set).  A local key frame that is not optimised
 * (fixed, or without an edge) comes back as the widened input.  num_fixedKF = n_fixed + (a local key frame is fixed ? 1 : 0); zero
 * returns status ORBX_LBA_ABORTED with the outputs equal to the widened inputs (Optimizer.cc:1182), as does a problem without an
 * edge (ORBX_LBA_EMPTY) and params->stop != 0 (ORBX_LBA_STOPPED, the test of pbStopFlag at :1429).
 *
 * Deliberate differences from the reference:
 *  - pbStopFlag cannot interrupt a running optimisation: a chain of launches is not interruptible.  The flag is honoured where
 *    the reference tests it before optimising, and max_iterations (the reference passes 10, :1433) bounds the work instead.
 *  - LinearSolverEigen factors the reduced system by a sparse Cholesky under a fill-reducing ordering; the device factors it
 *    densely in key-frame order.  Both are exact factorisations: results differ by rounding (tests/lba_cases.py measures it).
 *  - KannalaBrandt8 key frames and the EdgeSE3ProjectXYZToBody edges of a two-camera rig (:1383-1423) have an entry of their
 *    own, orbx_local_bundle_adjustment_rig (below): here a key frame with model == ORBX_CAMERA_KB8 or camera2 != 0 is
 *    ORBX_E_BADARG.  The map-merge overload (:3567) is orbx_merge_bundle_adjustment (below).  Not built: the inertial variants
 *    and a batched entry.
 * Capacity: ORBX_LBA_MAX_LOCAL optimised key frames; fixed key frames, points and edges are bounded by int32 and memory. */
#define ORBX_LBA_MAX_LOCAL 128
#define ORBX_LBA_DONE 0      /* optimised */
#define ORBX_LBA_ABORTED 1   /* num_fixedKF == 0 */
#define ORBX_LBA_STOPPED 2   /* params->stop */
#define ORBX_LBA_EMPTY 3     /* no edge: g2o has nothing to optimise */
/* stop_reason of an optimised problem */
#define ORBX_LBA_STOP_ITERATIONS 0   /* max_iterations reached */
#define ORBX_LBA_STOP_QMAX 1         /* ten rejected trials in one iteration */
#define ORBX_LBA_STOP_RHO_ZERO 2     /* rho == 0 */
#define ORBX_LBA_STOP_SMALL_GAIN 3   /* three iterations in a row gained less than 1e-3 of their chi2 */
typedef struct orbx_lba_keyframe {
  float q[4];          /* Tcw: unit quaternion x y z w */
  float t[3];
  float fx, fy, cx, cy, bf;
  int32_t model;       /* ORBX_CAMERA_PINHOLE */
  int32_t fixed;       /* != 0: a fixed vertex */
  int32_t camera2;     /* != 0: the key frame has mpCamera2 (rejected) */
} orbx_lba_keyframe;   /* 60 bytes */
typedef struct orbx_lba_edge {
  int32_t kf;          /* index into keyframes */
  int32_t point;       /* index into points */
  float u, v;          /* mvKeysUn[leftIndex].pt */
  float u_right;       /* mvuRight[leftIndex]; < 0: monocular */
  float inv_sigma2;    /* mvInvLevelSigma2[octave] */
} orbx_lba_edge;       /* 24 bytes */
typedef struct orbx_lba_problem {
  const orbx_lba_keyframe* keyframes;   /* [n_local + n_fixed] */
  const float* points;                  /* [n_points][3] */
  const orbx_lba_edge* edges;           /* [n_edges] */
  int32_t n_local, n_fixed, n_points, n_edges;
} orbx_lba_problem;
typedef struct orbx_lba_params {
  int32_t max_iterations;   /* 1 .. 1000000; the reference's optimize(10) */
  int32_t stop;             /* *pbStopFlag at the time of the call */
  float lambda_init;        /* > 0: setUserLambdaInit; otherwise computed */
} orbx_lba_params;          /* 12 bytes */
typedef struct orbx_lba_result {
  double* poses;            /* out [n_local][7]: q (x y z w), t */
  double* points;           /* out [n_points][3] */
  uint8_t* erase;           /* out [n_edges]: the edge's (key frame, point) pair belongs to vToErase */
  double* chi2;             /* out [n_edges]: the chi2 the edge holds after the last trial */
  uint8_t* depth_positive;  /* out [n_edges]: isDepthPositive() at the final estimates */
  int32_t num_fixedKF, num_OptKF, num_MPs, num_edges;
  int32_t status;           /* ORBX_LBA_DONE ... */
  int32_t iterations;       /* solve() calls */
  int32_t trials;           /* Levenberg trials */
  int32_t stop_reason;      /* ORBX_LBA_STOP_* */
  double lambda;            /* the final lambda */
  double chi2_initial, chi2_final;   /* robust chi2 at the start and at the result */
} orbx_lba_result;
/* Everything is validated before a device is touched: null pointers and negative counts, finite poses (non-zero quaternion),
 * cameras (fx, fy > 0), points and observations, the pinhole model, no second camera, the fixed flags of the second group, edge
 * indices in range, edges grouped by ascending point without a repeated key frame, max_iterations in [1, 1000000], a finite lambda_init,
 * at most ORBX_LBA_MAX_LOCAL key frames to optimise.  Returns ORBX_OK (see result->status); valid arguments without a device
 * return ORBX_E_NODEVICE unless the call ends before the optimiser (aborted, stopped, empty).  Two calls on the same input
 * agree bit for bit. */
int orbx_local_bundle_adjustment(int device, const orbx_lba_problem* problem, const orbx_lba_params* params, orbx_lba_result* result);

/* ---- full bundle adjustment (Optimizer::GlobalBundleAdjustemnt) -------------------------------------------- */

/* Optimizer::BundleAdjustment (src/Optimizer.cc:47-372, behind GlobalBundleAdjustemnt: after the monocular initialisation,
 * src/Tracking.cc:2526, 20 iterations, robust; and in the thread that finishes a loop closure or a map merge,
 * src/LoopClosing.cc:2415, 10 iterations, not robust, mbStopGBA as its stop flag), one problem per call, on the device.  It is
 * the g2o problem of the local bundle adjustment -- Levenberg on BlockSolver_6_3 with the same two edge classes -- and runs
 * on the same kernel chain; see the section above for the arithmetic.  What differs:
 *  - the problem: orbx_lba_problem as it is.  Key frames in vpKFs order, fixed != 0 for the map's initial key frame, n_fixed may be
 *    0 (any key frame behind the first n_local must be fixed); points in vpMP order; edges grouped by ascending point.  poses
 *    comes back for all n_local + n_fixed key frames.
 *  - robust == 0: no robust kernel -- g2o then weighs with the information matrix alone (rho' = 1) and the chi2 is the plain
 *    sum; robust != 0: Huber with (float)sqrt(5.99) for monocular and (float)sqrt(7.815) for stereo edges (:129 writes 5.99,
 *    not the 5.991 of the local BA).
 *  - nothing aborts when no key frame is fixed (:116-127 has no such test): the damping carries the gauge, and a failed pivot
 *    is a rejected trial like any other.
 *  - no outlier classification and no erase flags (what :307-350 counts is read by nothing).
 *  - the linear solve.  A global map has hundreds of key frames: above the ORBX_LBA_MAX_LOCAL of the one-workgroup solver the
 *    reduced system is factored by a blocked LDLT spread over the chip (csrc/orbx_ba.hip), up to ORBX_BA_MAX_KF optimised key
 *    frames (6144 rows, 302 MB); beyond that a sparse method is the right tool.  solver: 0 chooses (the blocked one from
 *    ORBX_BA_BLOCKED_FROM_KF optimised key frames on), 1 forces the blocked solver, 2 forces the one-workgroup solver
 *    (ORBX_E_BADARG above ORBX_LBA_MAX_LOCAL).  Both are the same factorisation; their results differ by rounding.
 *  - stop_flag (pbStopFlag, may be NULL) is read by the host when the call starts, in front of the first trial and after every
 *    trial's status word -- where g2o asks terminate().  Set at the start: the widened inputs, ORBX_LBA_STOPPED, no device is
 *    touched.  Seen later: no further trial is enqueued and the result is the last accepted estimate, ORBX_LBA_STOPPED.
 * A key frame or point without an edge comes back as the widened input; a problem without an edge is ORBX_LBA_EMPTY.  status and
 * stop_reason take the ORBX_LBA_* values.  Deliberate difference: the reference writes back the estimate's quaternion after
 * Sophus renormalises the float cast; the library returns the double estimate and leaves the cast to the caller.
 * KannalaBrandt8 key frames and second cameras are rejected as in the local BA and go through orbx_bundle_adjustment_rig
 * (below); the map-merge overload of the local BA is orbx_merge_bundle_adjustment (below); the inertial variants are not built. */
#define ORBX_BA_MAX_KF 1024
/* solver == 0: fewer optimised key frames take the one-workgroup solver.  Measured on the MI355X (profiles/gba_bench.json, ms per
 * call of 5 trials, blocked against one workgroup): 3.05 / 2.77 at 47 optimised key frames, 4.06 / 4.58 at 63, 8.17 / 20.99 at 127. */
#define ORBX_BA_BLOCKED_FROM_KF 63
typedef struct orbx_ba_params {
  int32_t max_iterations;            /* 1 .. 1000000 */
  int32_t robust;                    /* != 0: Huber kernels */
  float lambda_init;                 /* > 0: setUserLambdaInit; otherwise computed */
  int32_t solver;                    /* 0 automatic, 1 blocked, 2 one workgroup */
  const volatile int32_t* stop_flag; /* may be NULL */
} orbx_ba_params;
typedef struct orbx_ba_result {
  double* poses;            /* out [n_local + n_fixed][7]: q (x y z w), t */
  double* points;           /* out [n_points][3] */
  double* chi2;             /* out [n_edges], may be NULL: the chi2 the edge holds after the last trial */
  int32_t status;           /* ORBX_LBA_DONE / ORBX_LBA_STOPPED / ORBX_LBA_EMPTY */
  int32_t iterations, trials, stop_reason;
  double lambda;
  double chi2_initial, chi2_final;
} orbx_ba_result;
/* Every check of orbx_local_bundle_adjustment, then at most ORBX_BA_MAX_KF key frames to optimise and a valid solver, all
 * before a device is touched.  Two calls on the same input agree bit for bit. */
int orbx_bundle_adjustment(int device, const orbx_lba_problem* problem, const orbx_ba_params* params, orbx_ba_result* result);
/* The blocked solver alone, for tests and measurements: A x = b for a symmetric positive definite row-major A [n][n] in double,
 * 1 <= n <= 6 * ORBX_BA_MAX_KF (only the lower triangle is read).  *ok = 0 when a pivot is <= 0 or not finite; x is then untouched. */
int orbx_ba_dense_solve(int device, int n, const double* A, const double* b, double* x, int32_t* ok);
/* The one-workgroup solver alone (the k_lba_solve of every local bundle adjustment, and of the full one below
 * ORBX_BA_BLOCKED_FROM_KF or under solver 2), for tests: the same contract, n a multiple of 6 in [6, 6 * ORBX_LBA_MAX_LOCAL]. */
int orbx_lba_dense_solve(int device, int n, const double* A, const double* b, double* x, int32_t* ok);

/* ---- bundle adjustments of KannalaBrandt8 key frames and two-camera rigs ------------------------------------ */

/* The two bundle adjustments above for the key frames they reject: a KannalaBrandt8 left camera and / or a second camera
 * (mpCamera2) whose observations become EdgeSE3ProjectXYZToBody edges (src/Optimizer.cc:1383-1423 in the local, :231-262 in the
 * full bundle adjustment).  The Levenberg state, reductions, Schur complement, both linear solvers, statuses, counters and result
 * structs are those of the sections above.  A problem is an orbx_lba_problem plus two parallel arrays:
 *  - cams[n_local + n_fixed], one orbx_lba_rig_camera per key frame: k[4], the left camera's KB8 mvParameters[4..7] (read when
 *    orbx_lba_keyframe::model == ORBX_CAMERA_KB8; fx fy cx cy stay in orbx_lba_keyframe); model2 and p2[8], the second camera's
 *    model (ORBX_CAMERA_NONE, ORBX_CAMERA_PINHOLE, ORBX_CAMERA_KB8) and mvParameters (pinhole reads the first four); trl_q / trl_t,
 *    GetRelativePoseTrl() as a quaternion x y z w and a translation, widened and normalised as SE3Quat(q, t) does.  The second
 *    camera is used when orbx_lba_keyframe::camera2 != 0; otherwise model2, p2 and Trl are only checked for a valid model2.
 *  - edge_camera[n_edges]: 0 an observation of the left camera, 1 of the second camera.
 * Edge classes.  Camera 0 on a pinhole key frame: the monocular or stereo edge of the sections above, the same arithmetic bit
 * for bit.  Camera 0 on a KB8 key frame: EdgeSE3ProjectXYZ with pCamera = KannalaBrandt8 -- error obs - project(T.map(Xw)), where
 * project(Vector3d) narrows theta and psi to float (KannalaBrandt8.cpp:48-66; the device rounds the double atan2 once to float),
 * Jacobians -projectJac R and -projectJac SE3deriv (KannalaBrandt8.cpp:149-184, all double).  Camera 1: EdgeSE3ProjectXYZToBody
 * (OptimizableTypes.cpp:189-212) -- error through (mTrl * T).map(Xw), the product normalised as SE3Quat::operator* does;
 * Xi = -projectJac(X_r) R(mTrl * T), Xj = -projectJac(X_r) R(mTrl) SE3deriv(X_l) with X_r = mTrl.map(T.map(Xw)); its camera is
 * the key frame's second one, pinhole or KB8.  KB8 and body edges have two rows, information inv_sigma2 I, the monocular Huber
 * delta and the gate 5.991; isDepthPositive() of a body edge is ((mTrl * T).map(X))[2] > 0.
 * A (key frame, point) pair carries at most two edges, one per camera; both add into the pair's Hpl block, and the Schur
 * complement takes every pair of edges of a point, the left x right terms on the diagonal included.
 * projectJac divides by x^2 + y^2: a point on the optical axis of a KB8 camera gives NaN Jacobians here as in the reference.
 * Deliberate difference: u_right >= 0 on a KB8 key frame is rejected.  The reference would build a pinhole
 * EdgeStereoSE3ProjectXYZ from the KB8 parameters there, which no real map produces.
 * A problem of pinhole key frames without second cameras returns the bits of the entries above. */
#define ORBX_CAMERA_NONE (-1)
typedef struct orbx_lba_rig_camera {
  float k[4];          /* left camera, KB8: mvParameters[4..7] */
  int32_t model2;      /* ORBX_CAMERA_NONE | ORBX_CAMERA_PINHOLE | ORBX_CAMERA_KB8 */
  float p2[8];         /* second camera: fx fy cx cy k1 k2 k3 k4 */
  float trl_q[4];      /* Trl: quaternion x y z w */
  float trl_t[3];
} orbx_lba_rig_camera;   /* 80 bytes */
typedef struct orbx_lba_rig_problem {
  orbx_lba_problem base;
  const orbx_lba_rig_camera* cams;   /* [n_local + n_fixed] */
  const uint8_t* edge_camera;        /* [n_edges] */
} orbx_lba_rig_problem;
/* Validation, before a device is touched, in this order.  Null pointers and negative counts (cams with any key frame, edge_camera
 * with any edge); max_iterations; lambda_init; per key frame in list order: the model (pinhole or KB8), the pose, the quaternion,
 * the camera parameters, finite KB8 k (KB8 key frames), a valid model2, camera2 != 0 with model2 == ORBX_CAMERA_NONE, the second
 * camera's parameters finite with fx, fy > 0, Trl finite, Trl's quaternion non-zero (the last four when camera2 != 0), the fixed
 * flag of the second group; the points; per edge in order: the indices, the grouping by point, edge_camera in {0, 1}, a key
 * frame repeated for the same camera within a point, finite observations, a camera-1 edge on a key frame without camera2, a
 * camera-1 edge with u_right >= 0, u_right >= 0 on a KB8 key frame; then the capacity (and, for the full one, the solver).
 * Valid arguments without a device return ORBX_E_NODEVICE unless the call ends before the optimiser.  Two calls on the same
 * input agree bit for bit. */
int orbx_local_bundle_adjustment_rig(int device, const orbx_lba_rig_problem* problem, const orbx_lba_params* params,
                                     orbx_lba_result* result);
int orbx_bundle_adjustment_rig(int device, const orbx_lba_rig_problem* problem, const orbx_ba_params* params, orbx_ba_result* result);

/* ---- map-merge bundle adjustment (the welding BA of LoopClosing::MergeLocal) ------------------------------- */

/* Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) (src/Optimizer.cc:3567-3994; the call site
 * src/LoopClosing.cc, inside MergeLocal, on the welding window), one problem per call, on the device.  It is the g2o problem of
 * the local bundle adjustment -- Levenberg on BlockSolver_6_3 with the same monocular and stereo edges -- on the same kernel
 * chain, run as TWO optimisations with a classification in between.  What differs from orbx_local_bundle_adjustment:
 *  - the problem: orbx_lba_problem as it is.  The n_local key frames of vpAdjustKF come first and must carry fixed == 0 -- the
 *    map's initial key frame stays free here (there is no GetInitKFid test) --, the n_fixed of vpFixedKF follow and must carry
 *    fixed != 0; a flag that contradicts its group is ORBX_E_BADARG.  n_fixed may be 0: nothing aborts without a fixed key frame.
 *    Points in the caller's order (the fixed key frames' points first, then the adjusted ones': :3612-3660), edges grouped by
 *    ascending point, each point's observations in the caller's order.
 *  - the Huber deltas are (float)sqrt(5.99) and (float)sqrt(7.815) (:3684 writes 5.99, as the full bundle adjustment does); the
 *    chi2 gates stay 5.991 and 7.815.
 *  - the rounds.  (1) optimize(iterations_first) over every edge with its robust kernel.  (2) Unless the stop flag is seen by
 *    then: every edge whose chi2 -- the one it holds after round one's LAST TRIAL, even a rejected one -- exceeds its gate, or
 *    whose depth at round one's estimates is not positive, goes to level 1 (result->level); every edge loses its robust kernel.
 *    (3) initializeOptimization(0), optimize(iterations_second): the level-0 edges only, from round one's estimates bit for bit
 *    (they never leave the device); a point or key frame without a level-0 edge takes no part and keeps round one's estimate;
 *    lambda is computed afresh (or is lambda_init again), ni returns to 2, every counter starts again.  (4) erase: chi2 over the
 *    gate or depth not positive, where a level-1 edge holds the chi2 of round one's last trial (round two never evaluates it)
 *    and every depth is taken at the FINAL estimates -- an edge put aside for its depth alone may come back un-erased.
 *    If every edge is put aside round two has nothing to optimise: rounds = 2, its counters are zero, round one's estimates
 *    come back.
 *  - stop_flag (pbStopFlag, may be NULL) is read as orbx_ba_params::stop_flag is.  Set when the call starts: the widened
 *    inputs, ORBX_LBA_STOPPED, rounds = 0, no device is touched.  Seen during round one or right behind it (the reference's
 *    bDoMore = false): no classification and no round two; rounds = 1, level is zero, the erase flags come from round one's
 *    robust edges, status ORBX_LBA_STOPPED.  Seen during round two: the last accepted estimate, rounds = 2, ORBX_LBA_STOPPED.
 * A key frame or point without any edge comes back as the widened input; a problem without an edge is ORBX_LBA_EMPTY with the
 * widened inputs.  Per-round fields are indexed by round - 1; a round that did not run holds zeros.  lambda_init > 0 is round
 * one's setUserLambdaInit (the reference sets none: pass 0; tests steer round one with it); round two computes its own.
 * orbx_merge_bundle_adjustment_rig takes KannalaBrandt8 left cameras (the reference builds these edges through pKF->mpCamera)
 * under the checks of orbx_local_bundle_adjustment_rig; this overload builds no EdgeSE3ProjectXYZToBody edge and never reads the
 * right index, so an edge with edge_camera == 1 is ORBX_E_BADARG.  A pinhole problem through it returns the bits of the plain entry.
 * Everything is validated before a device is touched: null pointers and negative counts, both iteration counts in
 * [1, 1000000], every check of the local entries, the fixed flags of both groups, (rig) no camera-1 edge, at most
 * ORBX_LBA_MAX_LOCAL key frames to optimise (MergeLocal hands over 25 + 25).  Valid arguments without a device return
 * ORBX_E_NODEVICE unless the call ends before the optimiser.  Two calls on the same input agree bit for bit.
 * Not built: the inertial MergeInertialBA. */
typedef struct orbx_mba_params {
  int32_t iterations_first;          /* 1 .. 1000000; the reference's optimize(5) */
  int32_t iterations_second;         /* 1 .. 1000000; the reference's optimize(10) */
  float lambda_init;                 /* > 0: round one's setUserLambdaInit; otherwise computed (the reference's) */
  int32_t reserved;                  /* 0 */
  const volatile int32_t* stop_flag; /* may be NULL */
} orbx_mba_params;
typedef struct orbx_mba_result {
  double* poses;            /* out [n_local][7]: q (x y z w), t */
  double* points;           /* out [n_points][3] */
  uint8_t* erase;           /* out [n_edges]: the edge's (key frame, point) pair belongs to vToErase */
  double* chi2;             /* out [n_edges]: the chi2 the edge holds at the end */
  uint8_t* depth_positive;  /* out [n_edges]: isDepthPositive() at the final estimates */
  uint8_t* level;           /* out [n_edges]: 1 = put aside after round one */
  int32_t status;           /* ORBX_LBA_DONE / ORBX_LBA_STOPPED / ORBX_LBA_EMPTY */
  int32_t rounds;           /* 0, 1 or 2 */
  int32_t n_level1;         /* edges put aside */
  int32_t reserved;
  int32_t iterations[2], trials[2], stop_reason[2];
  double lambda[2], chi2_initial[2], chi2_final[2];
} orbx_mba_result;
int orbx_merge_bundle_adjustment(int device, const orbx_lba_problem* problem, const orbx_mba_params* params, orbx_mba_result* result);
int orbx_merge_bundle_adjustment_rig(int device, const orbx_lba_rig_problem* problem, const orbx_mba_params* params,
                                     orbx_mba_result* result);
/* For tests: on != 0 makes the calling thread's following merge calls behave as if the stop flag were seen right behind round
 * one (a second thread cannot be timed to that point).  Returns the previous setting. */
int orbx_merge_ba_stop_after_first(int on);

/* ---- Sim3 pose graph (Optimizer::OptimizeEssentialGraph) --------------------------------------------------- */

/* The loop-closing Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections,
 * bFixScale) (src/Optimizer.cc:1530-1826; the call site src/LoopClosing.cc:1299, inside CorrectLoop), one graph per call, on the
 * device: g2o's Levenberg on BlockSolver_7_3 over VertexSim3Expmap vertices and EdgeSim3 edges, restated as a chain of kernels
 * (csrc/orbx_posegraph.hip), all arithmetic in double.
 *
 * The problem is a flat graph: vertices [n_vertices] = the estimates Siw (g2o::Sim3, the quaternion not normalised), fixed
 * [n_vertices] (!= 0: setFixed, the map's initial key frame; any number may be fixed), edges [n_edges] in the reference's order.
 * An edge holds vertex 0 = i, vertex 1 = j and the measurement Sji; its error is (Sji * S_i * S_j^-1).log()
 * (types_seven_dof_expmap.h:106-114), its information the identity, and it has no robust kernel.  Several edges may join the same
 * two vertices (a spanning-tree edge and a loop-connection edge, say), in either direction.  With fix_scale the seventh
 * component of every update is zeroed inside oplus (:64-65).  points / point_ref (optional): map point positions and the vertex
 * each is corrected through, -1: the point is neither read nor written (:1800-1822 for the others:
 * corrected_S[r].inverse().map(S[r].map(P)) in double with S the vertices as given, cast to float).
 *
 * Jacobians.  EdgeSim3 has no linearizeOplus: g2o differentiates numerically through oplusImpl by central differences with step
 * 1e-9, which leaves 1e-7 of rounding noise that no second implementation can reproduce.  The device does the same with step
 * 1e-6 (truncation about 1e-12, rounding about 1e-10, both relative).  A fixed vertex has no Jacobian.
 * The optimiser is optimization_algorithm_levenberg.cpp with the user's lambda_init (the reference: 1e-16, 20 iterations): a
 * trial solves (H + lambda I) x = b by the blocked LDLT of csrc/orbx_ba.hip over the dense 7 n_opt system, applies oplus,
 * takes rho = (chi2 - chi2_trial) / (sum x (lambda x + b) + 1e-3), accepts when rho > 0 and chi2_trial is finite (lambda *=
 * max(1/3, min(1 - (2 rho - 1)^3, 2/3)), ni = 2) and rejects otherwise (lambda *= ni, ni *= 2, the estimates restored); a failed
 * pivot is a rejected trial.  stop_reason takes the ORBX_LBA_STOP_* values: ten trials in one iteration (_QMAX), rho == 0, three
 * iterations in a row that gained less than 1e-3 of their starting chi2, or max_iterations.  Nothing aborts when no vertex is
 * fixed: the damping carries the gauge.  The rows of the system are the vertices that are not fixed and that an edge touches;
 * the others come back as given, bit for bit.
 * Early ends: a problem without an edge is ORBX_LBA_EMPTY, the outputs are the inputs and no device is touched.  A problem whose
 * every edge joins two fixed vertices has nothing to optimise: ORBX_LBA_DONE with the inputs, zero counters and the edges' chi2
 * (chi2_initial = chi2_final = their sum), which the device evaluates.
 * result->chi2 is every edge's chi2 at the returned estimate (the reference ends with computeActiveErrors, :1778).
 * Deliberate difference, as in the bundle adjustments: the library returns the double Sim3.  The [R | t / s] recovery of
 * :1789-1795 and its float cast belong to the caller.
 * Capacity: ORBX_PG_MAX_KF optimised vertices = floor(6 ORBX_BA_MAX_KF / 7), 6139 rows, inside the row count the blocked solver
 * is tested to (302 MB); more is ORBX_E_BADARG, and a sparse factorisation is the tool beyond.  Fixed vertices, edges and points
 * are bounded by int32 and memory.  Not built: the map-merge overload (:1828), OptimizeEssentialGraph4DoF and the inertial
 * variants; any number of fixed vertices and any edge list are accepted, so the merge overload is a second gather. */
#define ORBX_PG_MAX_KF 877
typedef struct orbx_pg_edge {
  int32_t i, j;              /* vertex 0, vertex 1 */
  orbx_sim3_pose Sji;        /* the measurement */
} orbx_pg_edge;              /* 72 bytes */
typedef struct orbx_pg_problem {
  const orbx_sim3_pose* vertices;
  const uint8_t* fixed;      /* [n_vertices] */
  int32_t n_vertices;
  const orbx_pg_edge* edges;
  int32_t n_edges;
  int32_t fix_scale;         /* bFixScale */
  const float* points;       /* [n_points][3], may be NULL with n_points == 0 */
  const int32_t* point_ref;  /* [n_points] vertex index, or -1 */
  int32_t n_points;
} orbx_pg_problem;
typedef struct orbx_pg_params {
  int32_t max_iterations;    /* 1 .. 1000000; the reference: 20 */
  double lambda_init;        /* finite and > 0; the reference: 1e-16 */
} orbx_pg_params;
typedef struct orbx_pg_result {
  orbx_sim3_pose* vertices;  /* out [n_vertices] */
  float* points;             /* out [n_points][3], may be NULL: no point is corrected */
  double* chi2;              /* out [n_edges], may be NULL */
  int32_t status;            /* ORBX_LBA_DONE / ORBX_LBA_EMPTY */
  int32_t iterations, trials, stop_reason;
  double lambda;
  double chi2_initial, chi2_final;
} orbx_pg_result;
/* All arguments are validated before a device is touched, in this order: null pointers and negative counts; max_iterations;
 * lambda_init; per vertex finite values, s > 0 and a non-zero quaternion; per edge the indices in [0, n_vertices), i != j and the
 * measurement as a vertex; per point point_ref in [-1, n_vertices) and, where it is not -1, a finite position; at most
 * ORBX_PG_MAX_KF vertices to optimise.  Valid arguments without a device return ORBX_E_NODEVICE unless the problem has no edge.
 * One upload and one download per call; two calls on the same input agree bit for bit.  Returns ORBX_OK (see result->status). */
int orbx_optimize_pose_graph(int device, const orbx_pg_problem* problem, const orbx_pg_params* params, orbx_pg_result* result);
/* For tests: per edge the error [n_edges][7] and, where jacobians is not NULL, both Jacobians [n_edges][2][7][7] (vertex i, then
 * vertex j; rows = error components; zero for a fixed vertex) at the given vertices, as the optimiser's first linearisation
 * computes them.  The problem is validated as above without the capacity; points are not read. */
int orbx_pose_graph_evaluate(int device, const orbx_pg_problem* problem, double* errors, double* jacobians);

/* ---- new map points (local mapping)------------------------------------------------------------------- */

/* The per-match geometry of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:504-707), which consumes the match list of
 * ORBmatcher::SearchForTriangulation: ray parallax and stereo parallax (:579-601), the choice between
 * GeometricTools::Triangulate (src/GeometricTools.cc:48-73) and KeyFrame::UnprojectStereo (src/KeyFrame.cc:756-773) (:607-624),
 * the depth signs (:631-635), the two chi-square reprojection gates (:638-685), the zero-distance, far-point and
 * scale-consistency gates (:688-707).  One kernel, one candidate per lane, float arithmetic in the reference's expression order
 * (doubles where the reference promotes: the 0.9996 / 0.9998 parallax thresholds, invz = 1.0 / z, 5.991 * sigma2, 7.8 * sigma2).
 *
 * Deliberate differences from the reference:
 *  - Triangulate's null vector of the float 4 x 4 comes from null_vector4 (double arithmetic on the float matrix, shared with the
 *    fisheye association and orbx_search_for_triangulation_rig) instead of Eigen::JacobiSVD<Matrix4f>: points agree to float
 *    rounding, accept / reject decisions unless a gated quantity lies within rounding noise of its threshold.
 *  - `if (i > 0 && CheckNewKeyFrames()) return` (:459) stays with the caller, who chooses how many neighbours a call gets.
 *  - MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth (:720-722) stay on the host.
 *
 * One camera of a key frame: its model, parameters (fx fy cx cy, then k0..k3 for KB8), pose Tcw (top three rows, row-major) and
 * centre Ow (GetPose / GetCameraCenter, or GetRightPose / GetRightCameraCenter). */
typedef struct orbx_np_camera {
  int32_t model;        /* ORBX_CAMERA_PINHOLE | ORBX_CAMERA_KB8 */
  float p[8];
  float kb8_precision;  /* KannalaBrandt8::precision (KB8 only) */
  float Tcw[12];
  float Ow[3];
} orbx_np_camera;       /* 100 bytes */
/* What CreateNewMapPoints reads of a key frame.  Single camera (n_cameras = 1, n_left = -1): kps = mvKeysUn, kps_raw = mvKeys
 * (read by UnprojectStereo only; NULL = kps), u_right / depth = mvuRight / mvDepth (both NULL: monocular).  Two cameras
 * (n_cameras = 2): kps = mvKeys | mvKeysRight, n_left = NLeft, cam[1] = the right camera; u_right / depth are not read (bStereo is
 * false for every feature, :516,526).  scale_factors / level_sigma2 = mvScaleFactors / mvLevelSigma2 (nlevels entries). */
typedef struct orbx_np_keyframe {
  orbx_np_camera cam[2];
  int32_t n_cameras;
  int32_t n_left;
  int32_t n;            /* features */
  int32_t nlevels;
  float mb;
  int32_t reserved;
  const orbx_keypoint* kps;
  const orbx_keypoint* kps_raw;
  const float* u_right;
  const float* depth;
  const float* scale_factors;
  const float* level_sigma2;
} orbx_np_keyframe;     /* 272 bytes */
typedef struct orbx_np_params {
  float mbf;              /* mpCurrentKeyFrame->mbf: used for BOTH key frames' stereo residual (:654,677) */
  int32_t inertial;       /* mbInertial: parallax threshold 0.9996 instead of 0.9998 */
  int32_t far_points;     /* mbFarPoints */
  float th_far;           /* mThFarPoints */
  float ratio_factor;     /* 1.5f * mpCurrentKeyFrame->mfScaleFactor (:451) */
  int32_t monocular;      /* mbMonocular: which baseline test skips a neighbour (orbx_create_new_map_points only) */
  int32_t only_stereo, coarse, check_orientation;  /* SearchForTriangulation's (orbx_create_new_map_points only; the call site
                                                      passes false, bCoarse, false) */
} orbx_np_params;         /* 36 bytes */
/* Status of one feature of key frame 1, in the reference's order of exits. */
#define ORBX_NP_CREATED 0
#define ORBX_NP_LOW_PARALLAX 1   /* :622-624 no stereo and very low parallax */
#define ORBX_NP_TRIANGULATE 2    /* Triangulate returned false (w == 0) */
#define ORBX_NP_UNPROJECT 3      /* UnprojectStereo returned false (z <= 0) */
#define ORBX_NP_Z1 4
#define ORBX_NP_Z2 5
#define ORBX_NP_REPROJ1 6
#define ORBX_NP_REPROJ2 7
#define ORBX_NP_ZERO_DIST 8
#define ORBX_NP_FAR 9
#define ORBX_NP_SCALE 10
#define ORBX_NP_NO_MATCH 255
/* One pair of key frames and a caller-supplied match list matches12[kf1->n] (idx2 or -1, as the searches return it; one feature
 * of key frame 2 may appear several times).  Outputs per idx1: status (above), x3d [n][3] (the point wherever one was computed,
 * i.e. status 0 or >= 4; zeros otherwise), point_stereo = bPointStereo.  The two key frames are both single-camera or both
 * two-camera.  Validated before a device is touched: octaves inside [0, nlevels), match indices inside [-1, n2), finite poses
 * and camera parameters.  Returns the number of points created (status 0) or a negative error. */
int orbx_triangulate_matches(int device, const orbx_np_keyframe* kf1, const orbx_np_keyframe* kf2, const int32_t* matches12,
                             const orbx_np_params* params, uint8_t* status, float* x3d, uint8_t* point_stereo);
/* The SearchForTriangulation arguments of a key frame that orbx_np_keyframe does not hold: mFeatVec as CSR, mDescriptors,
 * has_map_point (see orbx_search_for_triangulation). */
typedef struct orbx_np_bow {
  const uint32_t* node_ids;
  const int32_t* node_start;
  const uint32_t* feature_idx;
  const uint8_t* desc;
  const uint8_t* has_map_point;
  int32_t n_nodes;
  int32_t reserved;
} orbx_np_bow;            /* 48 bytes */
typedef struct orbx_np_neighbour {
  orbx_np_keyframe kf;
  orbx_np_bow bow;
  float ep[2], F12[9];    /* as orbx_search_for_triangulation takes them */
  float median_depth;     /* pKF2->ComputeSceneMedianDepth(2) (read when params->monocular) */
} orbx_np_neighbour;      /* 368 bytes */
#define ORBX_NP_MAX_NEIGHBOURS 30
/* The neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:458-727) for single-camera key frames (monocular,
 * rectified stereo, RGB-D): everything is uploaded once; per neighbour that passes the baseline test (:466-478, evaluated on the
 * host in float: baseline < pKF2->mb, or baseline / median_depth < 0.01 when monocular) the kernels of
 * orbx_search_for_triangulation and then the geometry above run on one stream.  A point created with neighbour i sets
 * has_map_point1[idx1] on the device (AddMapPoint, :717), which the search of neighbour i + 1 reads (:953): neighbour i of the
 * chain gives the bits of orbx_search_for_triangulation + orbx_triangulate_matches called with the flags updated on the host.
 * One download at the end: n_matches [K] (nmatches, -1 for a skipped neighbour), n_created [K], and rows of kf1->n entries per
 * neighbour -- matches12 [K][n], status [K][n], x3d [K][n][3], point_stereo [K][n] -- and has_map_point1_out [n], the final flags.
 * pKF2->AddMapPoint (:718) is the caller's: each neighbour's has_map_point is read only.  Returns the total number of points
 * created or a negative error. */
int orbx_create_new_map_points(int device, const orbx_np_keyframe* kf1, const orbx_np_bow* bow1, const orbx_np_neighbour* neighbours,
                               int n_neighbours, const orbx_np_params* params, int32_t* n_matches, int32_t* n_created,
                               int32_t* matches12, uint8_t* status, float* x3d, uint8_t* point_stereo, uint8_t* has_map_point1_out);


/* ---- key-frame database (place recognition) -------------------------------------------------------------------------------
 * ORB_SLAM3::KeyFrameDatabase (src/KeyFrameDatabase.cc) resident on the device: add / erase / clear / clearMap (:37-97),
 * DetectRelocalizationCandidates (:742-856) and DetectNBestCandidates (:612-740).  The BoW vector of every key frame lies in a
 * slot of a forward store (no inverted file); a query scores all slots at once.  Candidate lists, common-word counts, scores
 * and accumulated scores are those of the reference bit for bit:
 *  - the order of lKFsSharingWords is the order of (smallest word id shared with the query, sequence number of the add);
 *  - the score is DBoW2::L1Scoring::score(query, key frame), the sequential double sum in ascending word id, narrowed to float;
 *  - the covisibility accumulation adds the score a neighbour HOLDS: this query's if the neighbour passed the 0.8 word gate,
 *    otherwise what the last query of the same flavour that scored it left (0 after add), as the reference's mRelocScore /
 *    mPlaceRecognitionScore members do.  The two flavours keep separate scores.
 * What stays with the caller: key frames are ints (mnId) and maps are ints (Map::mnId); the ten best covisible key frames of a
 * key frame (GetBestCovisibilityKeyFrames(10)) are handed over with orbx_kfdb_set_covisibles whenever UpdateConnections changes
 * them, and belong to the database entry (erase drops them); bad key frames are erased (KeyFrame::SetBadFlag does); bad maps and
 * the query's connected key frames are per-call lists.  Calls on one database must not overlap. */
typedef struct orbx_kfdb orbx_kfdb;
/* Optional per-query records of a detect call, in the order of the reference's lScoreAndMatch (every key frame that passed
 * the word gate).  Arrays hold `cap` entries per query ([n_frames][cap] for the batched entry), n_scored / max_common_words one
 * per query; any pointer may be NULL.  n_scored may exceed cap: only the first cap records are written then. */
typedef struct orbx_kfdb_details {
  int32_t cap;
  int32_t* n_scored;
  int32_t* max_common_words;
  int32_t* kf_id;          /* the scored key frame */
  int32_t* common_words;   /* mnRelocWords / mnPlaceRecognitionWords */
  float* score;            /* si */
  float* acc_score;        /* accScore */
  int32_t* best_kf_id;     /* pBestKF */
} orbx_kfdb_details;
/* A database for up to max_keyframes key frames of up to max_words_per_keyframe words each (12 bytes of device memory per
 * word) on the vocabulary's device.  ORBX_E_UNSUPPORTED for a vocabulary whose scoring is not L1_NORM (0).  _create_sized takes
 * the two facts the database needs from a vocabulary: its number of words and its scoring type. */
int orbx_kfdb_create(const orbx_vocabulary* voc, int max_keyframes, int max_words_per_keyframe, orbx_kfdb** out);
int orbx_kfdb_create_sized(int device, int n_vocabulary_words, int scoring, int max_keyframes, int max_words_per_keyframe,
                           orbx_kfdb** out);
void orbx_kfdb_destroy(orbx_kfdb* db);
int orbx_kfdb_size(const orbx_kfdb* db);   /* key frames in the database, or a negative error */
/* Measurement aid (tools/bench_kfdb.py): on > 0 brackets the device work of every following detect call -- stage 1, the tails
 * and the copy back -- with two events on the database's stream, on = 0 stops, on < 0 leaves the setting.  last_ms (may be NULL)
 * receives the elapsed time of the last bracketed call, -1 before the first. */
int orbx_kfdb_profile(orbx_kfdb* db, int on, float* last_ms);
/* KeyFrameDatabase::add with pKF->mBowVec as host arrays: strictly ascending word ids below the vocabulary's word count
 * (ORBX_E_BADARG otherwise, and for kf_id < 0 or already present); ORBX_E_CAPACITY when the database is full or n_words exceeds
 * max_words_per_keyframe.  The key frame's stored scores start at 0 and its covisible list is empty. */
int orbx_kfdb_add(orbx_kfdb* db, int kf_id, int map_id, const uint32_t* word_ids, const double* word_values, int n_words);
/* The same with the BoW vector of image `image` of the handle's last orbx_bow_transform_batch, copied device to device. */
int orbx_kfdb_add_from_batch(orbx_kfdb* db, orbx_extractor* ex, int image, int kf_id, int map_id);
int orbx_kfdb_erase(orbx_kfdb* db, int kf_id);      /* ORBX_E_BADARG when absent */
int orbx_kfdb_clear(orbx_kfdb* db);
int orbx_kfdb_clear_map(orbx_kfdb* db, int map_id); /* returns the number of key frames removed */
/* best10 [n][10], -1 padded: GetBestCovisibilityKeyFrames(10) of key frames kf_ids[0..n) (all in the database, else
 * ORBX_E_BADARG and nothing changes).  Listed ids that are not in the database are ignored by the queries until they are. */
int orbx_kfdb_set_covisibles(orbx_kfdb* db, int n, const int32_t* kf_ids, const int32_t* best10);
/* DetectRelocalizationCandidates(F, pMap): the query's BoW vector (host arrays, ascending, at most 8192 words) and map.
 * candidates[0 .. min(*n, cap)) = vpRelocCandidates; *n is the full count, ORBX_E_CAPACITY when it exceeds cap. */
int orbx_kfdb_detect_relocalization_candidates(orbx_kfdb* db, const uint32_t* word_ids, const double* word_values, int n_words,
                                               int map_id, int32_t* candidates, int cap, int32_t* n, const orbx_kfdb_details* details);
/* The same for frames [first_image, first_image + n_frames) of the handle's last orbx_bow_transform_batch, read in place:
 * candidates [n_frames][cap], n [n_frames].  The results are those of n_frames single calls made in frame order. */
int orbx_kfdb_detect_relocalization_candidates_batch(orbx_kfdb* db, orbx_extractor* ex, int first_image, int n_frames,
                                                     const int32_t* map_ids, int32_t* candidates, int cap, int32_t* n,
                                                     const orbx_kfdb_details* details);
/* DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates): connected_ids = pKF->GetConnectedKeyFrames() (ids not in
 * the database are ignored), bad_map_ids = the maps whose IsBad() holds.  loop / merge hold n_candidates entries each. */
int orbx_kfdb_detect_n_best_candidates(orbx_kfdb* db, const uint32_t* word_ids, const double* word_values, int n_words, int map_id,
                                       const int32_t* connected_ids, int n_connected, const int32_t* bad_map_ids, int n_bad_maps,
                                       int n_candidates, int32_t* loop, int32_t* n_loop, int32_t* merge, int32_t* n_merge,
                                       const orbx_kfdb_details* details);


/* ---- measurement ------------------------------------------------------------------------------------ */

/* Per-kernel timing with HIP events recorded on the handle's own stream around every kernel launch (the
 * numbers bench.py's roofline object is built from).  Stages: */
#define ORBX_STAGE_RESIZE 0        /* 7 launches per extraction (one per pyramid level >= 1) */
#define ORBX_STAGE_DETECT 1
#define ORBX_STAGE_OCTREE 2
#define ORBX_STAGE_BLUR 3
#define ORBX_STAGE_SLOTS 4
#define ORBX_STAGE_DESCRIBE 5
#define ORBX_STAGE_STEREO_MATCH 6
#define ORBX_STAGE_STEREO_FILTER 7
#define ORBX_NUM_STAGES 8
/* on: 0 = off, 1 = bracket every kernel launch, 2 + s = bracket only the launches of stage s. */
int orbx_profile_enable(orbx_extractor* ex, int on);
/* Synchronises the stream, adds up the elapsed milliseconds / launch counts per stage since the last
 * collect and resets the log.  ms and launches hold ORBX_NUM_STAGES entries. */
int orbx_profile_collect(orbx_extractor* ex, double* ms, int32_t* launches);
const char* orbx_stage_name(int stage);
/* Pyramid geometry of the last configured image size: w/h per level (nlevels entries each) and the number
 * of FAST candidates / selected keypoints of image `image` per level (device counters, synchronises). */
int orbx_level_stats(orbx_extractor* ex, int image, int32_t* w, int32_t* h, int32_t* n_candidates,
                     int32_t* n_selected);

/* ---- test hooks -------------------------------------------------------------------------------------- */

/* Measurement aid: the shader clock while other work runs.  _start launches ONE wave on a private stream that spins for
 * spin_us microseconds between readings of s_memtime (shader cycles) and s_memrealtime (100 MHz); _finish waits for it and
 * returns cycles / ns = GHz of the shader clock domain during that interval (the probe handle is consumed).  bench.py
 * prints it as roofline.shader_clock_ghz instead of assuming the 2.4 GHz peak. */
int orbx_clock_probe_start(int device, int spin_us, void** probe);
int orbx_clock_probe_finish(void* probe, double* ghz);

/* Measurement aid: the device-copy rate the roofline fractions are ALSO quoted against.  Copies `bytes` (a multiple
 * of 16, >= 1 MiB) device to device `iters` times with a 16-byte-per-lane kernel and returns (bytes read + bytes written) / time in
 * GB/s -- the hardware guide measures 6.29 TB/s this way on MI355X (79 % of the 8 TB/s HBM3E peak). */
int orbx_copy_probe(int device, size_t bytes, int iters, double* gbps);

/* Runs the quadtree's host/device introsort replica (csrc/orbx_introsort.h) on the host: sorts n 64-bit
 * elements by their key bits 16..63, payload bits 0..15 ride along.  tests/ compare it with std::sort
 * (the tie order DistributeOctTree depends on, src/ORBextractor.cc:686). */
void orbx_debug_introsort(uint64_t* v, int n);
/* The wave-cooperative device version the quadtree kernel actually runs (n <= 4000). */
int orbx_debug_introsort_device(int device, uint64_t* v, int n);
/* The same with the workgroup named: nt = 64 is the single-wave form (introsort_wave), 128 / 256 / 512 the workgroup form
 * (introsort_block) with that many threads -- the three classes k_octree runs; the waves per round and the lanes per element of
 * the final rank (4 / 2 / 1, by 4 n <= nt and 2 n <= nt) depend on it.  (orbx_debug_introsort_device alternates 512 and 64
 * from call to call.) */
int orbx_debug_introsort_device_nt(int device, uint64_t* v, int n, int nt);
/* The small dense linear algebra of the geometric solvers (csrc/orbx_linalg.h), each function alone on n items of the caller's:
 * the kernels load an item, call the header's function and store what it returns.  in / out are packed arrays of items, doubles
 * unless stated.  out is read as well as written: where a function leaves an output untouched (jacobi_cs returning false, a
 * failed LDLT) the caller's value comes back.  Flags are written as 0.0 / 1.0.
 *   op                               in, per item                                  out, per item
 *   ORBX_LINALG_RCP64, _RSQRT64      x                                             rcp64(x) / rsqrt64(x)
 *   ORBX_LINALG_JACOBI_CS            alpha, beta, gamma                            c, s, returned flag
 *   ORBX_LINALG_SVD3                 A [3][3]                                      U [3][3], w [3], V [3][3]
 *   ORBX_LINALG_NULL_VECTOR4         A [4][4], float                               v [4], float
 *   ORBX_LINALG_LDLT6                H [21] (upper triangle, row-major), b [6]     x [6], returned flag
 *   ORBX_LINALG_LDLT6_DAMPED         H [21], b [6], lambda                         x [6], returned flag
 *   ORBX_LINALG_LDLT7                H [28], b [7], lambda                         x [7], returned flag
 *   ORBX_LINALG_NULL_VECTOR_SYM9     A [16][9]  (one wave per item: lane l holds   v [4][9]: the result as lanes 0, 17, 34 and 63
 *   ORBX_LINALG_NULL_VECTOR_SYM12    A [16][12]  row l & 15, as the call sites)    v [4][12]  of the wave hold it
 *   ORBX_LINALG_SUM16                v [64], one value per lane of a wave          sum16(v) [64], as every lane holds it
 *   ORBX_LINALG_HUBER                robust, chi2, delta                           rho0, rho1 (csrc/orbx_optim.h: huber)
 *   ORBX_LINALG_LM_STEP              lambda, ni, curChi, iniChi, iter, qmax,       the seven state fields, then accepted (0 / 1), next
 *                                    nbadR, tempChi, solveOk, scaleSum, maxIter    (0 retry, 1 next iteration, 2 stop), reason
 *                                    (csrc/orbx_optim.h: lm_step; integers as doubles)   (ORBX_LBA_STOP_*, -1 unless next is 2)
 * A null pointer, n outside [1, ORBX_LINALG_MAX_ITEMS] and an unknown op are ORBX_E_BADARG before any device is touched. */
#define ORBX_LINALG_RCP64 0
#define ORBX_LINALG_RSQRT64 1
#define ORBX_LINALG_JACOBI_CS 2
#define ORBX_LINALG_SVD3 3
#define ORBX_LINALG_NULL_VECTOR4 4
#define ORBX_LINALG_LDLT6 5
#define ORBX_LINALG_LDLT6_DAMPED 6
#define ORBX_LINALG_LDLT7 7
#define ORBX_LINALG_NULL_VECTOR_SYM9 8
#define ORBX_LINALG_NULL_VECTOR_SYM12 9
#define ORBX_LINALG_SUM16 10
#define ORBX_LINALG_HUBER 11
#define ORBX_LINALG_LM_STEP 12
#define ORBX_LINALG_OPS 13
#define ORBX_LINALG_MAX_ITEMS 65536
int orbx_debug_linalg(int device, int op, int n, const void* in, void* out);
/* The camera models and the SE3 / Sim3 maps of the solvers (csrc/orbx_kb8.h, orbx_kb8_edge.h, orbx_pose.h, orbx_sim3opt.h,
 * orbx_mlpnp.h), each function alone on n items of the caller's, one item per thread, as orbx_debug_linalg does for the linear
 * algebra.  Items of the three camera operations are floats, all others doubles; out is read as well as written.  Quaternions are
 * x y z w, a Pose is q [4], t [3], a Sim3 is q [4] (not normalised), t [3], s; matrices are row-major.  The model flag selects
 * KannalaBrandt8 (non-zero) or pinhole (zero); fixScale is 0.0 / 1.0.
 *   op                                       in, per item                                   out, per item
 *   ORBX_GEOM_CAM_PROJECT                    model flag, cam [8], X [3]        (float)      uv [2]
 *   ORBX_GEOM_CAM_UNPROJECT, _ROUNDED_TAN    model flag, cam [8], precision, u, v (float)   ray [3]
 *   ORBX_GEOM_KB8_PROJECT_D                  k [8] as floats (32 bytes), X [3] double       u, v
 *   ORBX_GEOM_KB8_PROJECT_JAC                the same (56 bytes = 7 doubles)                PJ [2][3]
 *   ORBX_GEOM_SE3_MAP                        Pose, X [3]                                    Y [3]
 *   ORBX_GEOM_SE3_COMPOSE                    Pose a, Pose b                                 Pose a * b
 *   ORBX_GEOM_QMUL                           a [4], b [4]                                   a * b [4]
 *   ORBX_GEOM_QROT                           q [4], v [3]                                   q * v [3]
 *   ORBX_GEOM_NORMALIZE_ROTATION             q [4]                                          q [4]
 *   ORBX_GEOM_QUAT_FROM_R                    R [3][3]                                       q [4]
 *   ORBX_GEOM_OPLUS                          x [6], Pose                                    Pose
 *   ORBX_GEOM_SIM3_EXP                       x [7]                                          Sim3
 *   ORBX_GEOM_SIM3_OPLUS                     x [7], fixScale, Sim3                          Sim3
 *   ORBX_GEOM_SO_INVERSE                     Sim3                                           qc [4], ti [3], si, Ri [3][3]
 *   ORBX_GEOM_RODRIGUES2ROT                  w [3]                                          R [3][3]
 *   ORBX_GEOM_ROT2RODRIGUES                  R [3][3]                                       w [3]
 * No operation indexes memory by a computed value and every loop is bounded (Newton's has 10 steps): NaN, inf and denormal items
 * are safe.  A null pointer, n outside [1, ORBX_GEOM_MAX_ITEMS] and an unknown op are ORBX_E_BADARG before any device is touched. */
#define ORBX_GEOM_CAM_PROJECT 0
#define ORBX_GEOM_CAM_UNPROJECT 1
#define ORBX_GEOM_CAM_UNPROJECT_ROUNDED_TAN 2
#define ORBX_GEOM_KB8_PROJECT_D 3
#define ORBX_GEOM_KB8_PROJECT_JAC 4
#define ORBX_GEOM_SE3_MAP 5
#define ORBX_GEOM_SE3_COMPOSE 6
#define ORBX_GEOM_QMUL 7
#define ORBX_GEOM_QROT 8
#define ORBX_GEOM_NORMALIZE_ROTATION 9
#define ORBX_GEOM_QUAT_FROM_R 10
#define ORBX_GEOM_OPLUS 11
#define ORBX_GEOM_SIM3_EXP 12
#define ORBX_GEOM_SIM3_OPLUS 13
#define ORBX_GEOM_SO_INVERSE 14
#define ORBX_GEOM_RODRIGUES2ROT 15
#define ORBX_GEOM_ROT2RODRIGUES 16
#define ORBX_GEOM_OPS 17
#define ORBX_GEOM_MAX_ITEMS 65536
int orbx_debug_geometry(int device, int op, int n, const void* in, void* out);

/* Shrinks (>= 320 entries) or restores (any larger value) the capacity of k_detect's LDS corner + survivor list so
 * that tests can force the paths natural images rarely reach: mid-cell flushes, the corner limit and the tile-scan
 * NMS behind it. */
void orbx_debug_set_detect_list_cap(int cap);
/* Test hook: != 0 forces k_octree's global-memory candidate path (normally taken only when one (image, level) has more
 * than 32 FAST candidates per thread of its block: 16384 with 512 threads); 0 restores the register-resident path. */
void orbx_debug_set_octree_global(int on);
/* Test hook of k_octree's workgroup size: 128, 256 or 512 = every level of every launch runs with workgroups of that many threads;
 * 0 (or anything else) restores the product: for batches the plan below, for a single frame 512 threads at every level.  With
 * 128 / 256 a level of more than 32 candidates per thread takes the global-memory candidate path; the results never change. */
void orbx_debug_set_octree_class(int nt);
/* k_octree's plan at this frame size (host only, no device): per level the class -- the threads of the level's workgroup that work
 * in a batch's launch: 128 / 256 / 512, non-increasing with the level; the launch has 512-thread workgroups and the waves past
 * the class end at once -- and the dynamic LDS bytes of that launch. */
int orbx_debug_octree_plan(const orbx_params* p, int width, int height, int32_t* nt_per_level, int32_t* lds_bytes_per_level);
/* Test hook of ComputeStereoMatches' two forms (src/Frame.cc:921-1084): calls with up to max_pairs pairs (and at most 4096
 * result slots per image) run the DIRECT form -- k_stereo_band selects its keypoints from the unsorted arrays itself, no
 * k_stereo_sort launch in front --, larger ones the row-sorted form.  Default 1 (the single-frame path); 0 = never; < 0
 * restores the default.  Environment: ORBX_STEREO_DIRECT_PAIRS. */
void orbx_debug_set_stereo_direct(int max_pairs);
/* Test hook of k_stereo_sort: what the row-sorted form of the handle's last association left for `pair` -- row_start
 * [2][height + 1] (CSR row tables of the left and the right eye), records [2][cap][4] ({x, y, octave | index << 8,
 * minr | maxr << 16}) and descriptors [2][cap][8], the first `cap` sorted slots of each eye.  Returns the slots per image of
 * the sorted arrays (cap may not exceed it).  The direct form does not write these arrays.  Synchronises the stream. */
int orbx_debug_stereo_sort(orbx_extractor* left, int pair, int32_t* row_start, uint32_t* records, uint32_t* descriptors, int cap);
/* Test hook of orbx_clahe's two apply forms (cv::CLAHE::apply, Examples/Stereo/stereo_tum_vi.cc:100,142-143): 1 (default) = one
 * workgroup per interpolation cell with the cell's table in LDS where the geometry allows it, 0 = the per-pixel table gathers
 * everywhere. */
/* Test hook of the batched, device-resident association paths (orbx_fisheye_stereo_match_batch, orbx_stereo_match_batch, the
 * batched matchers): overwrites image `image` of the handle's LAST extraction batch with n keypoints / descriptors given by the
 * caller (serial-order slots, mono_index = first lapping row), so that crafted sets -- ties, empty and one-row lapping areas,
 * sizes around the kernels' tile edges -- reach the kernels that normally only see extractor output.  Synchronises the stream. */
int orbx_debug_upload_results(orbx_extractor* ex, int image, const orbx_keypoint* kps, const uint8_t* desc, int n, int mono_index);
void orbx_debug_set_clahe_cell_kernel(int on);
/* Test hook of the pre-processing plans' two cv::remap forms (src/System.cc:294-295): 1 (default) = the source footprint of
 * every 128 x 8 output tile staged through LDS (k_remap_lds) where the plan's maps allow it, 0 = the per-thread window
 * gathers (k_remap1) everywhere. */
void orbx_debug_set_remap_lds(int on);
/* The footprint table of k_remap_lds as orbx_preproc_create builds it for these maps (n_maps maps of out_h rows of map_stride
 * floats each, one behind the other): per map and 128 x 8 output tile -- entry ((map * tiles_x) + tile_x) * tiles_y + tile_y --
 * eight ints {x0a, y0, 16-byte pieces per row, rows, ceil(2^32 / pieces), 0, 0, 0}: the source rectangle
 * [x0a, x0a + 16 * pieces) x [y0, y0 + rows) the workgroup stages.  Host only: touches no device and works without one.
 * Returns 1 when a table was built (n_maps * tiles_x * tiles_y entries copied to table), 0 when the plan would keep k_remap1
 * (a tile needs more than 256 pieces, src_w < 32 or src_w % 16 != 0; table untouched), ORBX_E_CAPACITY when cap (in ints) is
 * too small (table untouched), ORBX_E_BADARG on bad arguments.  tiles_x / tiles_y (may be NULL) receive the tile grid. */
int orbx_debug_remap_footprints(const float* map_x, const float* map_y, ptrdiff_t map_stride, int out_w, int out_h, int src_w,
                                int src_h, int n_maps, int32_t* table, int cap, int32_t* tiles_x, int32_t* tiles_y);
/* The tables that replace the fronts of k_detect and k_resize, as orbx_extractor_configure builds them for a width x height
 * frame and these parameters.  Host only: touches no device and works without one.
 *   cells: one record of 16 dwords per FAST cell, in the order (level, cell row, cell column):
 *     {iniX | iniY << 16, rw | rh << 16, flags | level << 8 | level width << 16, level pitch, byte offset of the ROI in an image's
 *      pyramid block, entry offset of the cell's candidate slots, slots, qpr | dq << 8 | rq << 16, 64 * whole-row rounds, 16-byte
 *      pieces of the score tile, lanes of the last round (2 dwords), threshold patterns of a row's last quad (2 dwords), 1 / qpr as
 *      a float, 0};  flags: 1 = rejected cell (every other field but level and width is 0), 2 = wide tile loader, 4 = level 0.
 *   tiles: per level >= 1, eight dwords per 256 x 16 destination tile (row-major) -- {first x-table entry, x0 | rows << 16,
 *     rb | nrows << 16, cb | ndw << 16, flags (1 = straight-line loader, 2 = every footprint dword inside its source row), byte
 *     offset of the tile's first row in the level, tile row, 0} --, then per tile row and wave 4 x {b0 | b1 << 16, byte offsets of the
 *     row's two source rows in the horizontal pass's output (512 bytes per footprint row, relative to rb), 0}.
 * info: {cell records, dwords of the tile table, LDS tile pitch of k_detect, its rows}.  cells / tiles may be NULL (sizes only);
 * ORBX_E_CAPACITY when a cap (in dwords) is too small. */
int orbx_debug_front_tables(const orbx_params* p, int width, int height, uint32_t* cells, int cells_cap, uint32_t* tiles,
                            int tiles_cap, int32_t info[4]);
/* The lane tables of k_resize_stream (the batched path's pyramid kernel for the levels k_resize_tail does not fuse: one-wave
 * workgroups, a lane per destination quad) as orbx_extractor_configure builds them for a width x height frame, for strips of
 * `quads` quads (32 or 64).  Host only: touches no device and works without one.  Per level >= 1 and strip, three blocks of `quads`
 * entries of four dwords, one entry per lane: {v_perm selectors of the quad's four columns: byte of S[sx] | 0x0c000c00 | byte of
 * S[sx + 1] << 16 within the lane's 8 loaded bytes}, {a0 | a1 << 16 of the four columns}, {byte offset of the lane's 8-byte load
 * in a source row, 4 * quad (the first destination column; 0xFFFFFFFF for a lane past the level's last quad, which repeats its
 * entries), 0, 0}.  level_off[ORBX_MAX_LEVELS] receives each level's first dword, -1 for level 0 and for a level that cannot
 * stream (a quad's source bytes span more than 8, or its source level is narrower than 8 pixels: it stays with k_resize).
 * Returns the dwords of the tables; lanes may be NULL (size and offsets only); ORBX_E_CAPACITY when lanes_cap (in dwords) is too
 * small. */
int orbx_debug_resize_stream_tables(const orbx_params* p, int width, int height, int quads, uint32_t* lanes, int lanes_cap,
                                    int32_t* level_off);
/* Test hook of k_resize_stream: builds levels 1 .. nlevels - 1 of n_images frames in device memory (any byte address for kernel
 * 1; row_pitch >= w) into the handle's pyramid with ONE kernel for every level -- kernel 1 = k_resize_stream with strips of `quads`
 * quads (32 / 64, 0 = what the batched path uses) and bands of `band` destination rows (0 = likewise), whatever the batch size;
 * kernel 0 = the tiled k_resize (4-byte aligned frames and pitches) -- and synchronises.  orbx_pyramid_download then returns the
 * levels.  Changes no setting of the handle: its extractions launch what they launched before.  ORBX_E_UNSUPPORTED when a level
 * cannot stream. */
int orbx_debug_resize_stream(orbx_extractor* ex, const uint8_t* d_images, int n_images, int w, int h, ptrdiff_t row_pitch,
                             ptrdiff_t image_pitch, int kernel, int quads, int band);
/* What a pre-processing plan decided at creation and what its LAST enqueue (orbx_preproc_run / _run_device,
 * orbx_extract_batch_raw_device) launched, from the expressions that pick the launch:
 *   info[0] k_remap_lds table built (0 / 1)          info[1] single-channel resize fast path prepared (0 / 1)
 *   info[2] remap form: 2 = k_remap_lds, 1 = k_remap1, 0 = k_remap      info[3] resize form: 1 = plain (the pyramid's k_resize),
 *   0 = generic          info[4] CLAHE read its source with dword loads (srcVec4, 0 / 1)
 *   info[5] 16-pixel segments per row of the gray pass (0 = the per-pixel kernel only)
 *   info[6] frames of the last enqueue (0 = none yet)                  info[7] 0
 * info[2..5] are -1 for a stage that is not part of the plan or has not run. */
int orbx_debug_preproc_plan(const orbx_preproc* pp, int32_t info[8]);
/* Test hook of the pyramid's fused small-level launches (k_resize_tail: up to three consecutive levels of
 * ComputePyramid, src/ORBextractor.cc:1108-1145, per launch).  first_level: -1 = the library's policy, 0 = no fusion (every
 * level through k_resize), >= 2 = fuse from that level on; max_levels / band_rows: levels per launch and rows of the last
 * level per workgroup (<= 0: defaults).  Applies to handles (re)configured afterwards, i.e. to the next image SIZE a handle
 * sees.  orbx_debug_resize_plan reports the fused segments of the handle's current size (returns their number). */
void orbx_debug_set_resize_tail(int first_level, int max_levels, int band_rows);
int orbx_debug_resize_plan(const orbx_extractor* ex, int32_t* first_level, int32_t* n_levels, int32_t* n_bands, int cap);
/* Test tap of k_detect: with enable != 0 every following extraction also writes, per pyramid level, the FAST score
 * (cornerScore, 0 = not a corner) of every detectable pixel at iniThFAST -- the corner set of cv::FAST BEFORE non-max
 * suppression (src/ORBextractor.cc:810-815).  orbx_debug_score_level copies one level (w x h bytes) to the host.
 * tests/test_pin_skimage.py compares it with scikit-image's independent segment test. */
int orbx_debug_score_map(orbx_extractor* ex, int enable);
int orbx_debug_score_level(orbx_extractor* ex, int image, int level, uint8_t* dst, ptrdiff_t dst_stride);
/* The device's sinf / cosf of the descriptor steering (computeOrbDescriptor, src/ORBextractor.cc:106-107: libm cosf / sinf;
 * csrc/orbx_sincos.h restates glibc's two x86-64 ifunc variants): evaluates n angles (radians, host arrays) with the FMA
 * (fused == 1) or the SSE2 variant (fused == 0), or with k_describe's own branch-free restatement of the FMA variant
 * (fused == 2: glibc_sincosf_sel, csrc/orbx_describe.hip -- the form the product runs; the other two are its definition).  tests/
 * compare all three with the host's libm bit for bit. */
int orbx_debug_sincos(int device, const float* angles, int n, int fused, float* sin_out, float* cos_out);
/* The device's cv::fastAtan2 of IC_Angle (src/ORBextractor.cc:98) in the branch-free form k_describe calls (fast_atan2_sel): n
 * pairs (y[i], x[i]) from host arrays, degrees to out.  ORBX_E_BADARG (NULL array, n < 0) before any device is touched;
 * ORBX_E_NODEVICE without a GPU. */
int orbx_debug_fast_atan2(int device, const float* y, const float* x, int n, float* out);
/* k_describe's launch plan for a batch of n_images width x height frames, exactly as the launch computes it (host only, no
 * device): out[0] = nk, the selected slots of one (image, level) a wave walks; out[1] = tasks, the workgroups per image;
 * out[2] = magic (as uint32: j / tasks == umulhi(j, magic) for every flat workgroup index j < n_images * tasks; 0 = no XCD
 * remap); out[3 + l] = first task of level l (INT32_MAX past the last level), ORBX_MAX_LEVELS entries. */
int orbx_debug_describe_plan(const orbx_params* p, int width, int height, int n_images, int32_t* out);
/* Test hook of the memory the one-shot entries recycle.  Every one of them lays its inputs, scratch and outputs out in one
 * block of a per-device pool that caches hipMalloc blocks in power-of-two size classes and hands them back as they are, and
 * uploads its inputs through a per-thread page-locked staging buffer of which only the items' own bytes are rewritten.  A
 * kernel that read a byte before anything of the same call wrote it would see what an EARLIER call left there.  This hook
 * lets a test decide what that is.  All three operations run under the pool's mutex, on `device`'s pool:
 *   ORBX_SCRATCH_STATS  out[0] = cached blocks, out[1] = cached bytes, out[2] = blocks taken from the pool so far,
 *                       out[3] = how many of those came from the cache (the others were allocated)
 *   ORBX_SCRATCH_FILL   waits for the device, sets every cached block to `byte` (0..255) and waits again, sets the calling
 *                       thread's staging buffer, as far as it is allocated, to the same byte; out[0] = device bytes filled
 *   ORBX_SCRATCH_TRIM   waits for the device and frees every cached block (out may be NULL)
 * ORBX_E_BADARG (unknown operation, NULL out, byte outside 0..255, no such device) before any device is touched;
 * ORBX_E_NODEVICE without a GPU.  The two counters of STATS are the hook's only cost in a product call. */
#define ORBX_SCRATCH_STATS 0
#define ORBX_SCRATCH_FILL 1
#define ORBX_SCRATCH_TRIM 2
int orbx_debug_scratch_pool(int device, int op, int byte, uint64_t* out);
/* The same for an extractor handle's own buffers, which only ever grow: waits for the handle's streams, then sets to `byte`
 * every device buffer that a call produces before it reads it -- candidate and selection lists, cell counts and prefixes,
 * slots, counts, keypoints, descriptors, the frame staging and the pyramid, the row-sorted stereo records, SAD distances,
 * uRight and depth, the fisheye association buffers, the bag-of-words buffers, the view lists of the device projections (a
 * search that reads them needs its projection call again), the score tap -- and the blurred levels, whose validity flag it
 * clears.  It leaves alone the tables of the configured frame size, what the caller uploaded (map, last frames, poses, lapping
 * areas) and the single-frame gather's arrival counter; csrc/orbx_host.h classifies every member.  No buffer moves, so a
 * captured pipeline stays valid.  Results of calls made before the hook are gone: downloads return the fill value. */
int orbx_debug_fill_work_buffers(orbx_extractor* ex, int byte);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H_ */
