/*
 * orbfe.h — C ABI of the MI355X-native ORB front-end (extractor + matchers).
 *
 * This is the drop-in seam for ORB-SLAM2's hot path as shipped in skaegy/ORBSLAM_MapSave.
 * Every entry point below replaces one reference interface; the replaced interface is cited
 * (file:line under the reference tree).  Plain C: no C++ types, no torch types, no exceptions.
 *
 * Conventions
 *   - Every function returns an int status (ORBFE_OK == 0, negative on error) unless it is a
 *     pure getter.  No function throws or aborts across the ABI.
 *   - "host" pointers are ordinary CPU memory; "_device" entry points take HIP device pointers
 *     and run asynchronously on the handle's stream (orbfe_set_stream); every other entry point
 *     is synchronous on return, matching the blocking semantics of the reference.
 *   - One handle is NOT reentrant (the reference ORBextractor keeps mvImagePyramid as instance
 *     state, ORBextractor.h:90).  Distinct handles are fully independent (own stream, own
 *     device buffers) and may be used from different threads concurrently.
 *   - The library never falls back to a CPU path: if no gfx950 device is usable, orbfe_create /
 *     orbfe_matcher_create fail with ORBFE_ERR_HIP.
 */
#ifndef ORBFE_H
#define ORBFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------- */
#define ORBFE_OK               0
#define ORBFE_ERR_ARG         -1   /* bad argument (NULL, negative size, ...)                   */
#define ORBFE_ERR_CAPACITY    -2   /* caller buffer too small; *n_out holds the required count  */
#define ORBFE_ERR_HIP         -3   /* HIP runtime error / no usable device                      */
#define ORBFE_ERR_UNSUPPORTED -4   /* input the reference handles only through UB (see DESIGN) */
#define ORBFE_ERR_NOMEM       -5   /* device allocation failed                                  */

/* ---- plain data types ----------------------------------------------------------------------- */

/* Extractor parameters: the five ctor arguments of ORBextractor (ORBextractor.h:56-57),
 * read from ORBextractor.{nFeatures,scaleFactor,nLevels,iniThFAST,minThFAST} (Tracking.cc:200-204). */
typedef struct orbfe_params {
    int32_t nfeatures;
    float   scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
} orbfe_params;

/* Layout-compatible with cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle, response, octave,
 * class_id.  Extractor output sets class_id = -1 exactly as cv::FAST does. */
typedef struct orbfe_keypoint {
    float   x, y;
    float   size;
    float   angle;
    float   response;
    int32_t octave;
    int32_t class_id;
} orbfe_keypoint;

/* Pixel formats of the frames handed to the colour entry points: the four cvtColor codes of
 * Tracking::GrabImageStereo / GrabImageRGBD / GrabImageMonocular (Tracking.cc:286-310,
 * 350-363, 409-422), chosen there by channels() and mbRGB (Camera.RGB, Tracking.cc:192). */
#define ORBFE_PIX_GRAY 0   /* CV_8UC1, no conversion                                          */
#define ORBFE_PIX_RGB  1   /* CV_8UC3, CV_RGB2GRAY  (mbRGB = 1)                               */
#define ORBFE_PIX_BGR  2   /* CV_8UC3, CV_BGR2GRAY  (mbRGB = 0)                               */
#define ORBFE_PIX_RGBA 3   /* CV_8UC4, CV_RGBA2GRAY                                           */
#define ORBFE_PIX_BGRA 4   /* CV_8UC4, CV_BGRA2GRAY                                           */

/* Zeroed rectangle of the human mask: rows [y0, y1) x cols [x0, x1) of an all-ones mask
 * (OpDetector::SkeletonSquareMask, DetectHumanPose.cpp:484-489). */
typedef struct orbfe_rect {
    int32_t x0, y0, x1, y1;
} orbfe_rect;

typedef struct orbfe_extractor  orbfe_extractor;
typedef struct orbfe_matcher    orbfe_matcher;
typedef struct orbfe_vocabulary orbfe_vocabulary;

/* ---- extractor ---------------------------------------------------------------------------- */

/* Replaces ORBextractor::ORBextractor (ORBextractor.cc:409-469).  `device` is the HIP ordinal;
 * `max_width`/`max_height`/`max_batch` size the device workspace (0 => 1920 x 1080 x 1, grown
 * on demand outside any captured region). */
orbfe_extractor* orbfe_create(const orbfe_params* params, int device, int max_width,
                              int max_height, int max_batch, int* status);
void orbfe_destroy(orbfe_extractor* h);

/* Which build of the reference's OpenCV 3.3 primitives the pixel arithmetic reproduces
 * (tests/golden/README.md).  ORBFE_ARITH_SCALAR: OpenCV's portable scalar
 * paths — resize FixedPtCast<int,uchar,22>, blur FixedPtCastEx, uncontracted rotation products.
 * ORBFE_ARITH_X86_SIMD (the default, what the reference's build.sh Release build computes on
 * x86-64, where SSE2 is always on): the SSE2 bodies of
 * VResizeLinearVec_32s8u (ORBextractor.cc:1123; ~18 % of the pixels of levels >= 1 differ
 * by 1 from the scalar path) and SymmColumnVec_32s8u (1089; ties rounded to even) with the
 * scalar tails past them, and the descriptor rotation FMA-contracted as GCC -O3 on an FMA host
 * builds computeOrbDescriptor (117-119).  The oct-tree's heap-address tie order (H2) cannot
 * be reproduced by any build and stays the documented creation-sequence rule.  Synchronizes
 * the handle's stream; applies to later calls. */
#define ORBFE_ARITH_SCALAR   0
#define ORBFE_ARITH_X86_SIMD 1
int orbfe_set_arithmetic(orbfe_extractor* h, int mode);
int orbfe_get_arithmetic(const orbfe_extractor* h);

/* The reference's compile-time constants as this library's kernels use them: PATCH_SIZE,
 * HALF_PATCH_SIZE, EDGE_THRESHOLD (ORBextractor.cc:71-73) and ORBmatcher::TH_HIGH, TH_LOW,
 * HISTO_LENGTH (ORBmatcher.cc:37-39).  Needs no device; for the known-answer check against the
 * reference text (tests/golden/constants_fixture.json). */
typedef struct orbfe_reference_constants {
    int32_t patch_size, half_patch_size, edge_threshold;
    int32_t th_high, th_low, histo_length;
} orbfe_reference_constants;
int orbfe_get_reference_constants(orbfe_reference_constants* out);

/* Getters — ORBextractor::GetLevels / GetScaleFactor / GetScaleFactors /
 * GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares
 * (ORBextractor.h:68-88).  Table outputs hold nlevels floats each; any may be NULL. */
int   orbfe_get_levels(const orbfe_extractor* h);
float orbfe_get_scale_factor(const orbfe_extractor* h);
int   orbfe_get_scale_tables(const orbfe_extractor* h, float* scale, float* inv_scale,
                             float* sigma2, float* inv_sigma2);
/* mnFeaturesPerLevel (ORBextractor.cc:434-445). */
int   orbfe_get_features_per_level(const orbfe_extractor* h, int32_t* out);
/* Per-frame keypoint capacity that can never overflow for this handle's params and ANY
 * supported input size (w, h <= 4096): the sum over levels of the oct-tree output bound
 * max(N_l + 4, 4 nIni_l, 20) at the widest aspect ratio (DESIGN.md "capacity"). */
int   orbfe_keypoint_capacity(const orbfe_extractor* h);
/* The same bound for one input size (w x hgt): what DistributeOctTree (ORBextractor.cc:538-762)
 * can return per level at that size, summed.  <= orbfe_keypoint_capacity(h); negative status
 * for an unsupported size. */
int   orbfe_keypoint_capacity_for(const orbfe_extractor* h, int w, int hgt);
/* orbfe_keypoint_capacity_for without a handle (host arithmetic only, no device): the bound
 * for extractor parameters `p` at w x hgt, so a caller can size its output slabs (e.g. config
 * 4's all-gathered descriptor slabs) before any extractor exists.  Negative status for bad
 * parameters or an unsupported size. */
int   orbfe_keypoint_capacity_params(const orbfe_params* p, int w, int hgt);

/* Replaces ORBextractor::operator()(image, mask, keypoints, descriptors)
 * (ORBextractor.h:64-66, ORBextractor.cc:1042-1108), called from Frame::ExtractORB
 * (Frame.cc:358-364, mask empty) and Frame::ExtractORBMask (Frame.cc:366-371).
 *   img   : w x h u8 gray, row stride `stride` bytes (CV_8UC1, asserted at ORBextractor.cc:1051)
 *   mask  : NULL for none, else w x h u8 with row stride `mask_stride`; pixels where mask==0
 *           are zeroed before the pyramid (Mat::copyTo(dst, mask), ORBextractor.cc:1053)
 *   kps   : kps_cap keypoints out, level-major order (ORBextractor.cc:1079-1107)
 *   desc  : kps_cap x 32 bytes out, row i <-> kps[i]
 *   n_out : number of keypoints written.
 * Empty image (img==NULL or w==0 or h==0): returns ORBFE_OK and touches nothing
 * (ORBextractor.cc:1045-1046).  kps_cap too small: ORBFE_ERR_CAPACITY, *n_out = required. */
int orbfe_extract(orbfe_extractor* h, const uint8_t* img, int w, int hgt, size_t stride,
                  const uint8_t* mask, size_t mask_stride, orbfe_keypoint* kps, int kps_cap,
                  uint8_t* desc, int* n_out);

/* Zero-copy form of the same call for the tracking loop.  Frame::ExtractORB
 * (Frame.cc:358-364) hands operator() the cv::Mat that GrabImageMonocular's cvtColor just
 * produced (Tracking.cc:409-422); orbfe_extract copies it into the handle's pinned staging
 * buffer first.  Instead:
 *   orbfe_input_buffer   : the handle's pinned, device-mapped w x h u8 staging buffer (*buf,
 *                          row stride *stride bytes) — wrap it as cv::Mat(h, w, CV_8UC1, buf,
 *                          stride) and let cvtColor write the gray frame straight into it.
 *                          It is separate from the staging orbfe_extract copies into: no
 *                          other call writes or moves it, and it stays valid until an
 *                          orbfe_input_buffer for a larger w x h or orbfe_destroy on h.
 *   orbfe_extract_staged : operator() on that buffer (the GPU reads it in place).  With
 *                          kps_cap == 0 (kps, desc NULL) the outputs stay in the handle's pinned
 *                          output buffers and orbfe_staged_outputs returns them (*n_out is set).
 *   orbfe_staged_outputs : the last single-frame call's keypoints / descriptors (n of them), in
 *                          handle-owned memory valid until the next call on h.
 * Errors and capacity rules as orbfe_extract; orbfe_extract_staged without a buffer handed out
 * for at least w x h returns ORBFE_ERR_ARG. */
int orbfe_input_buffer(orbfe_extractor* h, int w, int hgt, uint8_t** buf, size_t* stride);
int orbfe_extract_staged(orbfe_extractor* h, int w, int hgt, orbfe_keypoint* kps, int kps_cap,
                         uint8_t* desc, int* n_out);
int orbfe_staged_outputs(const orbfe_extractor* h, const orbfe_keypoint** kps,
                         const uint8_t** desc, int* n);

/* Colour front-end: cvtColor(img, gray, CV_*2GRAY) of Tracking::GrabImage* (Tracking.cc:409-422
 * and the stereo / RGB-D twins) fused with Frame::ExtractORBMask -> operator()(gray, mask)
 * (Frame.cc:366-371, ORBextractor.cc:1053).  `pix` is an ORBFE_PIX_* format, `stride` the row
 * stride of img in bytes (>= w * channels).  The mask is given as a u8 plane (`mask`, NULL for
 * none) and/or as the zeroed rectangle `rect` (NULL for none) of OpDetector's square mask;
 * a pixel survives when both keep it.  rect with x1 < x0 or y1 < y0 (where the reference's
 * rowRange/colRange assert) returns ORBFE_ERR_UNSUPPORTED.  Gray values follow OpenCV's 8U
 * integer path.  Otherwise as orbfe_extract. */
int orbfe_extract_color(orbfe_extractor* h, const uint8_t* img, int pix, int w, int hgt,
                        size_t stride, const uint8_t* mask, size_t mask_stride,
                        const orbfe_rect* rect, orbfe_keypoint* kps, int kps_cap, uint8_t* desc,
                        int* n_out);

/* The human-mask rectangle from 25 OpenPose joints (x, y, score) — the bounding box of the
 * joints grown by 30 px and clamped to the image, exactly as OpDetector::SkeletonSquareMask
 * computes it (DetectHumanPose.cpp:453-489).  Host-only helper (no device work). */
int orbfe_human_mask_rect(const float* joints, int njoints, int w, int hgt, orbfe_rect* out);

/* Throughput form of orbfe_extract over n same-size frames (host buffers).  Frame f's
 * keypoints go to kps[f*kps_cap ...], descriptors to desc[f*kps_cap*32 ...], count n_out[f].
 * masks may be NULL (no masks) or an array of n pointers (entries may be NULL). */
int orbfe_extract_batch(orbfe_extractor* h, const uint8_t* const* imgs, int n, int w, int hgt,
                        size_t stride, const uint8_t* const* masks, size_t mask_stride,
                        orbfe_keypoint* kps, int kps_cap, uint8_t* desc, int32_t* n_out);

/* Device-resident throughput form: d_imgs holds n frames, frame f at d_imgs + f*frame_pitch,
 * rows `stride` bytes apart.  d_masks NULL or laid out like d_imgs.  Outputs are device
 * slabs laid out as in orbfe_extract_batch.  Asynchronous on the handle's stream.
 * kps_cap below orbfe_keypoint_capacity_for(h, w, hgt) returns ORBFE_ERR_CAPACITY before any
 * device work, so no frame is ever truncated; d_n_out[f] is frame f's keypoint count. */
int orbfe_extract_batch_device(orbfe_extractor* h, const uint8_t* d_imgs, int n, int w, int hgt,
                               size_t stride, size_t frame_pitch, const uint8_t* d_masks,
                               orbfe_keypoint* d_kps, int kps_cap, uint8_t* d_desc,
                               int32_t* d_n_out);

/* Device-resident colour form: frame f at d_imgs + f*frame_pitch in format `pix`; d_masks NULL
 * or n u8 planes (mask_stride, mask_frame_pitch); d_rects NULL or n device orbfe_rect.  Level 0
 * (the gray, masked image) is made by one fused kernel before the pipeline. */
int orbfe_extract_color_batch_device(orbfe_extractor* h, const uint8_t* d_imgs, int pix, int n,
                                     int w, int hgt, size_t stride, size_t frame_pitch,
                                     const uint8_t* d_masks, size_t mask_stride,
                                     size_t mask_frame_pitch, const orbfe_rect* d_rects,
                                     orbfe_keypoint* d_kps, int kps_cap, uint8_t* d_desc,
                                     int32_t* d_n_out);

/* Stream control: `hip_stream` is a hipStream_t (NULL => the handle's own stream, which is
 * non-blocking: it does not order against the legacy default stream).  To run on the device's
 * legacy default stream (handle 0 in frameworks that expose it, e.g. torch's default stream),
 * pass hipStreamLegacy ((void*)1); the same holds for the matcher and vocabulary handles. */
int orbfe_set_stream(orbfe_extractor* h, void* hip_stream);
int orbfe_synchronize(orbfe_extractor* h);

/* Per-kernel timing of the extraction pipeline: when enabled, a HIP event pair is recorded on
 * the handle's stream around every kernel launch.  orbfe_profile_read synchronizes the stream
 * and returns, per stage (ORBFE_STAGE_*), the summed duration in ms and the launch count since
 * the previous read.  Used by bench.py for the roofline figure; off by default.
 * enable: 0 off, 1 every stage, or ORBFE_PROFILE_STAGE(s) OR-ed together to time only those
 * stages (the other launches carry no events). */
#define ORBFE_PROFILE_STAGE(s) (2 << (s))
#define ORBFE_STAGE_MASK     0   /* K0: colour conversion + mask (level 0) */
#define ORBFE_STAGE_RESIZE   1
#define ORBFE_STAGE_FAST     2
#define ORBFE_STAGE_OCTREE   3
#define ORBFE_STAGE_BLUR     4
#define ORBFE_STAGE_DESCRIBE 5
#define ORBFE_STAGE_COUNT    6
int orbfe_profile(orbfe_extractor* h, int enable);
int orbfe_profile_read(orbfe_extractor* h, double* total_ms, int32_t* launches);

/* Which pyramid path an extraction of `nframes` frames at the extractor's current frame size
 * takes (the last extracted size; a test hook, no reference counterpart): ORBFE_PYR_PER_LEVEL
 * (resize2_kernel pairs / resize_kernel + resize_tail_kernel), ORBFE_PYR_BANDS
 * (pyramid_kernel); ORBFE_ERR_ARG before any extraction.  (Value 2, the rolling-band kernel of
 * rounds 4-5, was removed with that kernel and is never returned.) */
#define ORBFE_PYR_PER_LEVEL 0
#define ORBFE_PYR_BANDS     1
int orbfe_pyramid_path(const orbfe_extractor* h, int nframes);
/* How that extraction makes the small top levels (a test hook as well): ORBFE_TAIL_NONE (no
 * resize_tail_kernel launch: the band kernel, a batch below the tail's minimum, or no run of
 * top levels that fits), ORBFE_TAIL_GATHER (its horizontal pass by byte gathers: scale factors
 * without column-group tables, ORBFE_RESIZE_TABLE=0), ORBFE_TAIL_TABLE (on the column-group
 * tables). */
#define ORBFE_TAIL_NONE   0
#define ORBFE_TAIL_GATHER 1
#define ORBFE_TAIL_TABLE  2
int orbfe_pyramid_tail(const orbfe_extractor* h, int nframes);
/* Describe's matrix-core window blur, host side (a test hook as well; no device): the seven
 * blur taps of these parameters (taps7), the six constant MFMA fragments as the kernel loads
 * them (frags: 384 lanes x 16 bytes — H_0..H_2, lane n + 16 g, byte j = raw column 16 g + j ->
 * window column 16 s + n; then V_0..V_2, lane n + 16 g, byte j = 4 t + i = R row 16 t + 4 g + i
 * -> window row 16 u + n) and the constant bytes of the column pass's spare K slots j = 12..14
 * (pads: hi plane scalar, hi plane x86, lo plane scalar, lo plane x86; byte i <-> j = 12 + i).
 * ORBFE_ERR_UNSUPPORTED if a slot weight does not fit an i8 or a constant is not met exactly. */
int orbfe_describe_blur_fragments(const orbfe_params* p, int32_t* taps7, uint8_t* frags,
                                  uint32_t* pads);
/* Measurement hook: relaunch the stages in `stage_mask` (bits 1 << ORBFE_STAGE_*) of the most
 * recent extraction on its own buffers, `reps` times, asynchronously on the handle's stream
 * (outputs meaningful only for a full mask). */
int orbfe_debug_replay(orbfe_extractor* h, unsigned stage_mask, int reps);
/* Stage pipelining: later extraction calls on `h` run only the stages in `stage_mask` (bits
 * 1 << ORBFE_STAGE_*; 0 = all, the default).  A batch extracted in two calls on the same handle,
 * buffers and frames — stages up to the oct-tree, then describe — equals one full call; the
 * caller orders the calls (e.g. on two streams, so that one sub-batch's describe runs beside
 * another's FAST). */
int orbfe_set_stage_mask(orbfe_extractor* h, unsigned stage_mask);

/* Pyramid access — replaces the public member mvImagePyramid (ORBextractor.h:90) read by
 * stereo matching (Frame.cc:589, 679, 696).  Copies level `level` of frame `frame` of the
 * most recent extraction (interior pixels only, rows w bytes apart) into `out`
 * (out may be NULL to query w/h). */
int orbfe_get_level(orbfe_extractor* h, int frame, int level, uint8_t* out, int* w, int* hgt);

/* Stage probes of the most recent extraction, for parity tests against the oracle:
 * blurred level (GaussianBlur 7x7 sigma 2 REFLECT_101, ORBextractor.cc:1088-1089) and the
 * per-level FAST output before distribution (vToDistributeKeys, ORBextractor.cc:777-828;
 * coordinates relative to (16,16), response = FAST score). */
int orbfe_get_blurred_level(orbfe_extractor* h, int frame, int level, uint8_t* out, int* w,
                            int* hgt);
int orbfe_get_fast_keys(orbfe_extractor* h, int frame, int level, orbfe_keypoint* out, int cap,
                        int* n_out);

/* ---- stereo ------------------------------------------------------------------------------ */

/* Frame::ComputeStereoMatches (Frame.cc:584-756), called by the stereo Frame ctor right after
 * the two extractions (Frame.cc:78-103).  kl/dl: mvKeys + mDescriptors of the left image (nl,
 * distorted keypoints as extracted); kr/dr: mvKeysRight + mDescriptorsRight (nr).  The pyramids
 * read are mpORBextractorLeft/Right->mvImagePyramid: frame `frame` of the most recent
 * extraction of `left` / `right` (same image size and scale parameters).  bf = mbf, b = mb.
 * Writes mvuRight / mvDepth (nl floats each, -1 = no match).  Inputs on which the reference
 * indexes vRowIndices out of range or trips a rowRange/colRange assert return
 * ORBFE_ERR_UNSUPPORTED.  Synchronous; runs on left's stream after right's stream. */
int orbfe_compute_stereo_matches(orbfe_extractor* left, orbfe_extractor* right, int frame,
                                 const orbfe_keypoint* kl, const uint8_t* dl, int nl,
                                 const orbfe_keypoint* kr, const uint8_t* dr, int nr, float bf,
                                 float b, float* u_right, float* depth);

/* Device-resident batch form over frames 0..n-1 of the two handles' most recent
 * orbfe_extract*_batch_device calls: keypoint / descriptor / count slabs as those calls write
 * them (kps_cap keypoints per frame); u_right / depth are n x kps_cap floats.  The device frames
 * the extractions read must still be valid (level 0 is read in place).  Asynchronous on left's
 * stream (ordered after right's stream); orbfe_stereo_status reports UB inputs afterwards. */
int orbfe_compute_stereo_matches_device(orbfe_extractor* left, orbfe_extractor* right, int n,
                                        const orbfe_keypoint* d_kl, const uint8_t* d_dl,
                                        const int32_t* d_nl, const orbfe_keypoint* d_kr,
                                        const uint8_t* d_dr, const int32_t* d_nr, int kps_cap,
                                        float bf, float b, float* d_u_right, float* d_depth);
/* Synchronizes left's stream; ORBFE_OK or ORBFE_ERR_UNSUPPORTED for the last stereo call. */
int orbfe_stereo_status(orbfe_extractor* left);

/* ---- RGB-D ------------------------------------------------------------------------------- */

/* The two depth image types Tracking::GrabImageRGBD is fed (Tracking.cc:345-368). */
#define ORBFE_DEPTH_U16 0   /* CV_16UC1                                                        */
#define ORBFE_DEPTH_F32 1   /* CV_32FC1                                                        */

/* Frame::ComputeStereoFromRGBD (Frame.cc:759-780) with the depth conversion in front of it
 * (imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor), Tracking.cc:367-368) fused: `depth` is
 * the raw w x hgt plane (rows `stride` bytes apart), depth_factor = mDepthMapFactor after
 * Tracking.cc:236-240.  Only the n pixels under the keypoints are read and scaled; the converted
 * plane is never made.  keys = mvKeys (distorted, as extracted: the lookup position, truncated
 * toward zero, row = y, column = x); keys_un = mvKeysUn (its x gives mvuRight = x - bf / d), or
 * NULL for mvKeysUn = mvKeys (the k1 == 0 branch of Frame::UndistortKeyPoints).  bf = mbf.
 * Writes mvuRight / mvDepth (n floats each; -1 where d > 0 fails).  A keypoint whose row or
 * column lies outside the image (or is NaN) reads out of bounds in the reference: it gets
 * -1 / -1, every other keypoint its values, and the call returns ORBFE_ERR_UNSUPPORTED.
 * When `depth` is the buffer of the depth-buffer call below, the kernel gathers from it in
 * place; any other pointer is copied in first.  Synchronous on h's stream. */
int orbfe_compute_stereo_from_rgbd(orbfe_extractor* h, const void* depth, int depth_type, int w,
                                   int hgt, size_t stride, float depth_factor,
                                   const orbfe_keypoint* keys, const orbfe_keypoint* keys_un,
                                   int n, float bf, float* u_right, float* depth_out);

/* The depth twin of the input buffer: device-mapped pinned memory of hgt rows, *stride bytes
 * apart, that the caller's grabber writes the raw depth plane into.  It stays valid until a
 * larger one is asked for or the handle is destroyed. */
int orbfe_depth_buffer(orbfe_extractor* h, int w, int hgt, int depth_type, void** buf,
                       size_t* stride);

/* Device-resident batch form over the keypoint / count slabs the batch extractions write
 * (kps_cap keypoints per frame, d_n[f] of them valid): d_depth holds n_frames raw planes
 * frame_pitch bytes apart; d_keys_un may be NULL; d_u_right / d_depth_out are n_frames x kps_cap
 * floats, slots at and past d_n[f] are left alone.  Asynchronous on h's stream; the status call
 * below reports out-of-image keypoints afterwards. */
int orbfe_compute_stereo_from_rgbd_device(orbfe_extractor* h, int n_frames, const void* d_depth,
                                          int depth_type, int w, int hgt, size_t stride,
                                          size_t frame_pitch, float depth_factor,
                                          const orbfe_keypoint* d_keys,
                                          const orbfe_keypoint* d_keys_un, const int32_t* d_n,
                                          int kps_cap, float bf, float* d_u_right,
                                          float* d_depth_out);
/* Synchronizes h's stream; ORBFE_OK or ORBFE_ERR_UNSUPPORTED for the last RGB-D call. */
int orbfe_rgbd_status(orbfe_extractor* h);

/* ---- matchers ------------------------------------------------------------------------------- */

/* Frame data the matchers read.  Mirrors the Frame members the reference matchers touch:
 * mvKeysUn (x, y, octave, angle), mDescriptors, mvuRight, image bounds mnMin/MaxX/Y and
 * mfGridElementWidthInv/HeightInv (Frame.cc:212-213), mvScaleFactors.  The 64 x 48 grid of
 * Frame::AssignFeaturesToGrid (Frame.cc:341-356) is rebuilt from keys_un inside the call. */
typedef struct orbfe_frame_view {
    int32_t               n;
    const orbfe_keypoint* keys_un;        /* n                                                 */
    const uint8_t*        desc;           /* n x 32                                            */
    const float*          u_right;        /* n, or NULL for monocular (all -1)                 */
    float                 min_x, max_x, min_y, max_y;
    float                 grid_w_inv, grid_h_inv;
    const float*          scale_factors;  /* nlevels                                           */
    int32_t               nlevels;
} orbfe_frame_view;

/* Per-MapPoint tracking scratch (MapPoint.h:106-111) + the getters SearchByProjection reads. */
typedef struct orbfe_mappoint_view {
    int32_t        m;
    const uint8_t* track_in_view;  /* mbTrackInView                                         */
    const uint8_t* is_bad;         /* isBad()                                               */
    const float*   proj_x;         /* mTrackProjX                                           */
    const float*   proj_y;         /* mTrackProjY                                           */
    const float*   proj_xr;        /* mTrackProjXR                                          */
    const int32_t* pred_level;     /* mnTrackScaleLevel                                     */
    const float*   view_cos;       /* mTrackViewCos                                         */
    const uint8_t* desc;           /* GetDescriptor(), m x 32                               */
    const int32_t* n_obs;          /* Observations()                                        */
} orbfe_mappoint_view;

/* Camera + pose for the last-frame projection matcher (ORBmatcher.cc:1341-1379). Row-major
 * 3x4 [R|t] world->camera. */
typedef struct orbfe_camera {
    float fx, fy, cx, cy, bf, b;   /* mbf and mb (= mbf/fx, Frame.cc:225)                    */
} orbfe_camera;

orbfe_matcher* orbfe_matcher_create(int device, int* status);
void orbfe_matcher_destroy(orbfe_matcher* m);
int  orbfe_matcher_set_stream(orbfe_matcher* m, void* hip_stream);

/* ORBmatcher::DescriptorDistance (ORBmatcher.cc:1650-1666): dist[i] = Hamming(a_i, b_i). */
int orbfe_hamming(orbfe_matcher* m, const uint8_t* a, const uint8_t* b, int n, int32_t* dist);

/* Brute-force Hamming (config 3, no single reference function): for each query the best and
 * second-best distance over all references with the first-wins update rule of
 * ORBmatcher.cc:102-114 (best/second start at 256).  Host buffers. */
int orbfe_bf_match(orbfe_matcher* m, const uint8_t* q, int nq, const uint8_t* r, int nr,
                   int32_t* best_idx, int32_t* best_dist, int32_t* second_dist);
/* Device-resident batched form: `nb` independent (query-set, reference-set) problems;
 * problem b reads d_q + b*q_pitch (nq_b = d_nq[b] rows) against d_r + b*r_pitch
 * (nr_b = d_nr[b] rows) and writes d_out + b*nq_cap*3 as (best_idx, best, second) triples.
 * Reference sets hold fewer than 65536 rows: the kernels search the first 65,535 rows of a
 * larger set (indices are 16-bit fields of the ranking keys). */
int orbfe_bf_match_batch_device(orbfe_matcher* m, const uint8_t* d_q, size_t q_pitch,
                                const int32_t* d_nq, int nq_cap, const uint8_t* d_r,
                                size_t r_pitch, const int32_t* d_nr, int nb, int32_t* d_out);

/* Timing of orbfe_bf_match_batch_device launches (dispatch-bound HIP events, as
 * orbfe_profile): summed ms and launch count since the previous read.  Stage 0 is the
 * brute-force match kernels, stage 1 the expansion of a batch-shared reference set (r_pitch 0)
 * into matrix-core fragments; orbfe_matcher_profile_read reports stage 0,
 * orbfe_matcher_profile_read_stages fills ORBFE_MATCHER_STAGES entries.  Either read resets. */
#define ORBFE_MATCHER_STAGES 2
int orbfe_matcher_profile(orbfe_matcher* m, int enable);
int orbfe_matcher_profile_read(orbfe_matcher* m, double* total_ms, int32_t* launches);
int orbfe_matcher_profile_read_stages(orbfe_matcher* m, double* total_ms, int32_t* launches);

/* ORBmatcher::SearchForInitialization (ORBmatcher.cc:408-523), matcher built as
 * ORBmatcher(nnratio, check_ori) (Tracking.cc:843).  prev_matched: inout F1.n (x,y) pairs
 * (vbPrevMatched); matches12: out F1.n (vnMatches12). */
int orbfe_search_for_initialization(orbfe_matcher* m, float nnratio, int check_ori,
                                    const orbfe_frame_view* f1, const orbfe_frame_view* f2,
                                    float* prev_matched, int window, int32_t* matches12,
                                    int32_t* nmatches);

/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (ORBmatcher.cc:45-129).
 * frame_mp: inout F.n, id of the MapPoint held by each keypoint or -1 (F.mvpMapPoints);
 * frame_mp_obs: inout F.n, Observations() of that MapPoint.  A match writes
 * mp_ids[i] (or i when mp_ids is NULL) and mps->n_obs[i]. */
int orbfe_search_by_projection_local(orbfe_matcher* m, float nnratio,
                                     const orbfe_frame_view* f, int32_t* frame_mp,
                                     int32_t* frame_mp_obs, const orbfe_mappoint_view* mps,
                                     const int32_t* mp_ids, float th, int32_t* nmatches);

/* ORBmatcher::SearchByProjection(Frame& Cur, const Frame& Last, th, bMono)
 * (ORBmatcher.cc:1331-1473).  The last frame is given as its N_last keypoints (octave, angle
 * from last_keys), the world position/descriptor/Observations() of the MapPoint it holds
 * (last_mp_valid[i] == 0 <=> NULL), and mvbOutlier. Poses are row-major 3x4 world->camera. */
int orbfe_search_by_projection_last(orbfe_matcher* m, int check_ori,
                                    const orbfe_frame_view* cur, const float* tcw_cur,
                                    const orbfe_camera* cam, int32_t* frame_mp,
                                    int32_t* frame_mp_obs, int n_last,
                                    const orbfe_keypoint* last_keys,
                                    const uint8_t* last_mp_valid, const uint8_t* last_outlier,
                                    const float* last_mp_xyz, const uint8_t* last_mp_desc,
                                    const int32_t* last_mp_nobs, const int32_t* last_mp_ids,
                                    const float* tcw_last, float th, int mono,
                                    int32_t* nmatches);

/* Tracking::SearchLocalPoints (Tracking.cc:1403-1455) on device-resident data: for every local
 * map point that is neither bad (d_bad) nor already matched in the frame (d_skip[i] != 0 <=>
 * mnLastFrameSeen == mCurrentFrame.mnId), Frame::isInFrustum(pMP, viewing_cos_limit) with
 * MapPoint::PredictScale (Frame.cc:387-443, MapPoint.cc:633-642), then
 * ORBmatcher(nnratio).SearchByProjection(F, vpLocalMapPoints, th) (ORBmatcher.cc:45-129).
 * `frame` is a view whose keys_un / desc / u_right are DEVICE pointers (scale_factors stays a
 * host table).  Map-point arrays (xyz, normal n x 3; mfMinDistance / mfMaxDistance; descriptor
 * n x 32; Observations(); ids or NULL) are device arrays.  d_in_view receives mbTrackInView
 * (0 for skipped or bad points); d_frame_mp / d_frame_mp_obs are updated in place.
 * counts[0] = nmatches, counts[1] = nToMatch (host).  A predicted level outside the pyramid
 * returns ORBFE_ERR_UNSUPPORTED (such points are not matched).  Synchronous on return. */
int orbfe_search_local_points_device(orbfe_matcher* m, const orbfe_frame_view* frame,
                                     const float* tcw, const orbfe_camera* cam,
                                     float log_scale_factor, float viewing_cos_limit, int n_mp,
                                     const float* d_xyz, const float* d_normal,
                                     const float* d_min_dist, const float* d_max_dist,
                                     const uint8_t* d_desc, const int32_t* d_nobs,
                                     const uint8_t* d_bad, const uint8_t* d_skip,
                                     const int32_t* d_mp_ids, float nnratio, float th,
                                     int32_t* d_frame_mp, int32_t* d_frame_mp_obs,
                                     uint8_t* d_in_view, int32_t* counts);
/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (ORBmatcher.cc:45-129)
 * alone, on device-resident data: the isInFrustum outputs (mbTrackInView, mTrackProjX/Y/XR,
 * mnTrackScaleLevel, mTrackViewCos — Tracking.cc:1425-1438 computed them) are already in HBM.
 * `frame` as for orbfe_search_local_points_device (device keys_un / desc / u_right, host
 * scale_factors); every pointer in `d_mps` and d_mp_ids (or NULL) is a device pointer;
 * d_frame_mp / d_frame_mp_obs are updated in place; *nmatches (host).  A tracked point whose
 * predicted level is outside the pyramid returns ORBFE_ERR_UNSUPPORTED.  Synchronous. */
int orbfe_search_by_projection_local_device(orbfe_matcher* m, float nnratio,
                                            const orbfe_frame_view* frame, int32_t* d_frame_mp,
                                            int32_t* d_frame_mp_obs,
                                            const orbfe_mappoint_view* d_mps,
                                            const int32_t* d_mp_ids, float th, int32_t* nmatches);
/* Jacobi rounds the most recent SearchByProjection / SearchForInitialization resolution took
 * (diagnostics). */
int orbfe_matcher_last_rounds(const orbfe_matcher* m);
/* Calls of this matcher rerun because their candidate lists outgrew the device buffer (the
 * first attempt bounds every fill by the buffer and reads unfilled lists as empty; the rerun
 * uses the exact total) — diagnostics for the capacity tests. */
int orbfe_matcher_capacity_retries(const orbfe_matcher* m);

/* Frame::GetFeaturesInArea (Frame.cc:445-498) over the 64 x 48 grid of
 * Frame::AssignFeaturesToGrid / PosInGrid (Frame.cc:341-356, 500-510), exactly as every matcher
 * above builds and queries it — exported for the grid's parity tests.  Query q is
 * (x[q], y[q], r[q], min_level[q], max_level[q]); its candidates, in the reference's order (cell
 * column ix, then row iy, then insertion order), go to items[off[q] .. off[q + 1]).  off holds
 * nq + 1 entries (off[nq] = total).  wave != 0 runs the wave-per-query form
 * (SearchForInitialization, last-frame and keyframe SearchByProjection), wave == 0 the
 * thread-per-query form (local-map SearchByProjection).  total > items_cap: ORBFE_ERR_CAPACITY
 * with off filled and items untouched.  Synchronous; host buffers. */
int orbfe_features_in_area(orbfe_matcher* m, const orbfe_frame_view* f, int nq, const float* x,
                           const float* y, const float* r, const int32_t* min_level,
                           const int32_t* max_level, int wave, int32_t* off, int32_t* items,
                           int items_cap);

/* Relocalisation ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF,
 * const set<MapPoint*>& sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1475-1602), called by
 * Tracking::Relocalization with ORBmatcher(0.9, true), th/ORBdist = 10/100 and 3/64
 * (Tracking.cc:1664, 1723, 1737).  The keyframe is given as its n_kf map-point slots
 * (pKF->GetMapPointMatches(); kf_mp_valid[i] == 0 <=> NULL) with isBad(), sAlreadyFound
 * membership, world position (n_kf x 3), descriptor (n_kf x 32), mfMinDistance /
 * mfMaxDistance and the rotation angle pKF->mvKeysUn[i].angle.  frame_mp: inout cur->n ids
 * (-1 = NULL; a slot holding a point is never re-assigned); a match writes kf_mp_ids[i] (or i).
 * log_scale_factor = mfLogScaleFactor.  A predicted scale level outside the pyramid (where the
 * fork indexes mvScaleFactors out of range; MapPoint::PredictScale has no clamp) returns
 * ORBFE_ERR_UNSUPPORTED. */
int orbfe_search_by_projection_keyframe(orbfe_matcher* m, int check_ori,
                                        const orbfe_frame_view* cur, const float* tcw_cur,
                                        const orbfe_camera* cam, float log_scale_factor,
                                        int32_t* frame_mp, int n_kf, const float* kf_key_angle,
                                        const uint8_t* kf_mp_valid, const uint8_t* kf_mp_bad,
                                        const uint8_t* already_found, const float* kf_mp_xyz,
                                        const uint8_t* kf_mp_desc, const float* kf_mp_min_dist,
                                        const float* kf_mp_max_dist, const int32_t* kf_mp_ids,
                                        float th, int orb_dist, int32_t* nmatches);

/* ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>&, th) (ORBmatcher.cc:828-978, called by
 * LocalMapping::SearchInNeighbors, LocalMapping.cc:489, 514) and Fuse(KeyFrame* pKF, cv::Mat Scw,
 * const vector<MapPoint*>&, th, vpReplacePoint) (ORBmatcher.cc:980-1103, called by
 * LoopClosing::SearchAndFuse, LoopClosing.cc:597): the search half.  Everything either overload
 * computes up to bestIdx / bestDist reads only data that Replace / AddObservation / AddMapPoint
 * never change, so the search runs for all points at once and the caller applies the
 * GetMapPoint(bestIdx) branch afterwards, walking the points in order and re-evaluating the skip
 * test (isBad(), IsInKeyFrame / spAlreadyFound) against live state — identical to the
 * sequential loop (include/orbfe_orbslam.hpp ORBmatcher::Fuse does that walk).
 *   kf     : the keyframe's mvKeysUn, mDescriptors, mvuRight, image bounds, grid constants and
 *            mvScaleFactors; tcw its row-major 3x4 [R|t] world->camera pose.  For the Sim3
 *            overload the caller passes the normalised pose (R = sRcw / scw, t = tcw / scw,
 *            ORBmatcher.cc:989-992).
 *   inv_level_sigma2 : pKF->mvInvLevelSigma2, kf->nlevels floats (read in SE3 mode only).
 *   points : n_mp world positions (x 3), normals GetNormal() (x 3), mfMinDistance /
 *            mfMaxDistance (the 0.8 / 1.2 factors of Get*DistanceInvariance are applied
 *            inside) and descriptors (x 32).
 *   skip   : NULL or n_mp bytes; a point with skip[i] != 0 is not searched (the loop's
 *            `continue` at 849-853 / 1008-1009).
 *   mode   : ORBFE_FUSE_SE3 applies the chi-square tests of 917-941 (7.8 with mvuRight >= 0,
 *            5.99 otherwise); ORBFE_FUSE_SIM3 has none.
 * best_idx[i] = the keypoint with the smallest descriptor distance among the candidates of
 * KeyFrame::GetFeaturesInArea(u, v, th * mvScaleFactors[nPredictedLevel]) that pass the level
 * (and chi-square) tests, first in the reference's order on ties, if that distance is <= TH_LOW;
 * otherwise -1.  best_dist[i] (may be NULL) = that distance, 256 when no candidate survived.
 * *n_found = the number of points with best_idx >= 0.  A predicted scale level outside the
 * pyramid (where the fork indexes mvScaleFactors out of range) returns ORBFE_ERR_UNSUPPORTED;
 * such a point gets no match and every other point's result is valid.  Synchronous. */
#define ORBFE_FUSE_SE3  0
#define ORBFE_FUSE_SIM3 1
int orbfe_fuse_search(orbfe_matcher* m, const orbfe_frame_view* kf, const float* tcw,
                      const orbfe_camera* cam, float log_scale_factor,
                      const float* inv_level_sigma2, int n_mp, const float* mp_xyz,
                      const float* mp_normal, const float* mp_min_dist,
                      const float* mp_max_dist, const uint8_t* mp_desc, const uint8_t* skip,
                      float th, int mode, int32_t* best_idx, int32_t* best_dist,
                      int32_t* n_found);
/* Device-resident batched form, the shape of both call sites (every neighbour / corrected
 * keyframe against one shared point set): n_kf keyframes in pitched slabs — keyframe k's
 * keypoints at d_keys + k*keys_pitch (orbfe_keypoint units), descriptors at d_desc +
 * k*desc_pitch (bytes, a multiple of 16), mvuRight at d_u_right + k*kp_cap (d_u_right NULL:
 * monocular), d_n[k] keypoints (clipped to kp_cap; pitches below kp_cap keypoints / kp_cap * 32
 * bytes return ORBFE_ERR_ARG).  tcw is a HOST array of n_kf x 12 floats
 * (read before the call returns); the camera, image bounds, scale tables (host, nlevels <= 16)
 * and the n_mp points are shared by all keyframes.  d_skip: NULL or n_kf x n_mp bytes, one per
 * (keyframe, point).  Outputs d_best_idx / d_best_dist (may be NULL): n_kf x n_mp, keyframe k's
 * row at k*n_mp.  *d_status = 0, or ORBFE_ERR_UNSUPPORTED (a predicted level outside the
 * pyramid, as above).  All keyframes' grids are built by one launch and all pairs searched by
 * one launch per 40 keyframes; asynchronous on the matcher's stream. */
int orbfe_fuse_search_batch_device(orbfe_matcher* m, int n_kf, const orbfe_keypoint* d_keys,
                                   size_t keys_pitch, const uint8_t* d_desc, size_t desc_pitch,
                                   const float* d_u_right, int kp_cap, const int32_t* d_n,
                                   const float* tcw, const orbfe_camera* cam, float min_x,
                                   float max_x, float min_y, float max_y,
                                   const float* scale_factors, const float* inv_level_sigma2,
                                   int nlevels, float log_scale_factor, int n_mp,
                                   const float* d_xyz, const float* d_normal,
                                   const float* d_min_dist, const float* d_max_dist,
                                   const uint8_t* d_mp_desc, const uint8_t* d_skip, float th,
                                   int mode, int32_t* d_best_idx, int32_t* d_best_dist,
                                   int32_t* d_status);

/* Loop-closing ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw,
 * const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th)
 * (ORBmatcher.cc:293-406), called by LoopClosing::ComputeSim3 with ORBmatcher(0.75, true) and
 * th = 10 on the loop keyframe's covisible points (LoopClosing.cc:376).  Per point the tests are
 * those of Fuse's Sim3 overload (depth, KeyFrame::IsInImage, the 0.8 / 1.2 distance window, the
 * 60-degree viewing angle, MapPoint::PredictScale, KeyFrame::GetFeaturesInArea without a level
 * filter, octave in [lvl - 1, lvl]); the tail is greedy: a keypoint that holds a point before
 * the call, or that an earlier point of the list took, is passed over (378, 399), and the best
 * remaining candidate is accepted at a distance <= TH_LOW.
 *   kf, tcw, cam, log_scale_factor : as for orbfe_fuse_search in ORBFE_FUSE_SIM3 mode — tcw is
 *            the normalised [R|t] (R = sRcw / scw, t = tcw / scw, ORBmatcher.cc:302-305), which
 *            the caller computes (include/orbfe_orbslam.hpp does).
 *   points : n_mp world positions (x 3), normals (x 3), mfMinDistance / mfMaxDistance and
 *            descriptors (x 32), in vpPoints order.
 *   skip   : NULL or n_mp bytes: isBad() || spAlreadyFound.count(pMP) (320).  The reference
 *            builds that set once before the loop, so a point listed twice may match twice; the
 *            caller owns the flags and this call never changes them.
 *   mp_ids : NULL or n_mp ids; a match writes mp_ids[i] (or i) into the keypoint's slot.
 *   th     : the reference's int.
 *   kf_matched : inout kf->n ids (vpMatched, -1 = NULL), caller-owned.
 * *nmatches as returned.  A predicted scale level outside the pyramid returns
 * ORBFE_ERR_UNSUPPORTED; such a point gets no match and every other result is valid.
 * Synchronous; host buffers. */
int orbfe_search_by_projection_sim3(orbfe_matcher* m, const orbfe_frame_view* kf,
                                    const float* tcw, const orbfe_camera* cam,
                                    float log_scale_factor, int n_mp, const float* mp_xyz,
                                    const float* mp_normal, const float* mp_min_dist,
                                    const float* mp_max_dist, const uint8_t* mp_desc,
                                    const uint8_t* skip, const int32_t* mp_ids, int th,
                                    int32_t* kf_matched, int32_t* nmatches);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.cc:1105-1329),
 * called inside the RANSAC loop of LoopClosing::ComputeSim3 with ORBmatcher(0.75, true) and
 * th = 7.5 (LoopClosing.cc:324).  Each keyframe's map points are projected into the other
 * keyframe and matched to the keypoint with the smallest descriptor distance (the MapPoint's
 * descriptor against the keypoints', first in KeyFrame::GetFeaturesInArea order on ties, octave
 * in [lvl - 1, lvl], accepted at <= TH_HIGH); a pair is kept when both directions chose it.
 *   kf1, kf2 : the keyframes' mvKeysUn, mDescriptors, image bounds, grid constants and
 *            mvScaleFactors (nlevels <= 16 each; the two may differ).
 *   cam1   : pKF1's intrinsics, used in both directions (1108-1111).
 *   t1w, t2w : row-major 3x4 [R|t] world -> camera of the two keyframes.
 *   s12, s21 : row-major 3x4 [sR12|t12] and [sR21|t21] of lines 1122-1124, evaluated by the
 *            caller (include/orbfe_orbslam.hpp does).
 *   log_scale_factor1 / 2 : the keyframes' mfLogScaleFactor (the target's is the one read).
 *   per keyframe k, kfk->n entries each, caller-owned: searchk[i] != 0 <=> feature i holds a
 *            point that is not bad and is not already matched (vbAlreadyMatchedk, 1135-1145,
 *            filters sources only); xyzk (x 3), min_distk / max_distk and desck (x 32) of that
 *            point (entries with searchk[i] == 0 are not read for a result).
 * match12[i1] = idx2 for the agreeing pairs (1310-1326), -1 otherwise; vn_match1 / vn_match2
 * (each may be NULL) receive the two directions' own answers (vnMatch1, vnMatch2);
 * *n_found = nFound.  A predicted scale level outside the target's pyramid returns
 * ORBFE_ERR_UNSUPPORTED; that feature gets no match and every other result is valid.  Both
 * directions run in one kernel launch; synchronous; host buffers. */
int orbfe_search_by_sim3(orbfe_matcher* m, const orbfe_frame_view* kf1,
                         const orbfe_frame_view* kf2, const orbfe_camera* cam1, const float* t1w,
                         const float* t2w, const float* s12, const float* s21,
                         float log_scale_factor1, float log_scale_factor2,
                         const uint8_t* search1, const float* xyz1, const float* min_dist1,
                         const float* max_dist1, const uint8_t* desc1, const uint8_t* search2,
                         const float* xyz2, const float* min_dist2, const float* max_dist2,
                         const uint8_t* desc2, float th, int32_t* match12, int32_t* vn_match1,
                         int32_t* vn_match2, int32_t* n_found);

/* MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:483-548) for n_mp map points at once
 * (LocalMapping calls it for every new / fused point, LocalMapping.cc:268, 489).  The
 * descriptors of map point i's observations in non-bad keyframes, in mObservations order, are
 * rows obs_off[i] .. obs_off[i+1]-1 of obs_desc (obs_off has n_mp + 1 entries, < 65536
 * observations per point).  best[i] = the chosen row relative to obs_off[i] (least median
 * distance to the others, first on ties), -1 for a point without observations (mDescriptor
 * untouched); desc_out (n_mp x 32, may be NULL) receives mDescriptor. */
int orbfe_distinctive_descriptors(orbfe_matcher* m, int n_mp, const int32_t* obs_off,
                                  const uint8_t* obs_desc, int32_t* best, uint8_t* desc_out);
/* Device form of the same (asynchronous on the matcher's stream); d_desc_out may be NULL. */
int orbfe_distinctive_descriptors_device(orbfe_matcher* m, int n_mp, const int32_t* d_obs_off,
                                         const uint8_t* d_obs_desc, int32_t* d_best,
                                         uint8_t* d_desc_out);

/* Frame::isInFrustum (Frame.cc:387-443) + MapPoint::PredictScale (MapPoint.cc:633-642) over
 * m MapPoints: world pos (m x 3), normal (m x 3), mfMinDistance/mfMaxDistance.  Writes the
 * tracking scratch fields (mbTrackInView, mTrackProjX/Y/XR, mnTrackScaleLevel,
 * mTrackViewCos). log_scale_factor = mfLogScaleFactor (Frame.cc:185). */
int orbfe_is_in_frustum(orbfe_matcher* m, int n, const float* xyz, const float* normal,
                        const float* min_dist, const float* max_dist, const float* tcw,
                        const orbfe_camera* cam, float min_x, float max_x, float min_y,
                        float max_y, float log_scale_factor, float viewing_cos_limit,
                        uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr,
                        int32_t* pred_level, float* view_cos);

/* The close-point rule of an RGB-D / stereo frame and Frame::UnprojectStereo (Frame.cc:782-796).
 * ORBFE_CLOSE_SORTED is the loop Tracking::UpdateLastFrame (Tracking.cc:1059-1111) and
 * Tracking::CreateNewKeyFrame (Tracking.cc:1333-1392) share: the features with depth > 0 sorted
 * by (depth, index), visited until one lies beyond th_depth and more than min_points (the
 * reference's 100) have been visited.  ORBFE_CLOSE_ALL is Tracking::StereoInitialization
 * (Tracking.cc:764-779): every feature with depth > 0 in index order, all created, has_point
 * not read. */
#define ORBFE_CLOSE_SORTED 0
#define ORBFE_CLOSE_ALL    1
/* Most features with depth > 0 one frame may hold. */
#define ORBFE_CLOSE_MAX_KEPT 8192

/* keys_un = mvKeysUn, depth = mvDepth, has_point[i] = mvpMapPoints[i] && Observations() >= 1
 * (the fact bCreateNew, Tracking.cc:1086-1092 / 1362-1369, and nMap, 1261-1263, read; may be
 * NULL with ORBFE_CLOSE_ALL), n features.  cam: fx, fy, cx, cy.  rwc_ow: mRwc row-major (9) then
 * mOw (3), the products of Frame::UpdatePoseMatrices.  scale_factors = mvScaleFactors (nlevels,
 * at most 16).
 * Writes order[0..*n_visited): the feature indices the loop visits, in visiting order;
 * create[j]: visit j makes a new MapPoint; xyz[3j..]: UnprojectStereo(order[j]) where create[j]
 * (zeros elsewhere); max_dist[j] / min_dist[j]: mfMaxDistance / mfMinDistance of the Frame-form
 * MapPoint constructor (MapPoint.cc:298-305) where create[j] (zeros elsewhere; both may be
 * NULL).  Entries at and past *n_visited are left alone; the arrays hold n entries.
 * *n_total / *n_map: nTotal / nMap of Tracking::NeedNewKeyFrame (Tracking.cc:1256-1265) over the
 * whole frame, in either mode.  More than ORBFE_CLOSE_MAX_KEPT features with depth > 0 return
 * ORBFE_ERR_CAPACITY with nothing written.  A created visit whose octave lies outside
 * [0, nlevels) indexes mvScaleFactors out of range: its max_dist / min_dist are -1, the other
 * visits are intact, and the call returns ORBFE_ERR_UNSUPPORTED. */
int orbfe_close_points(orbfe_matcher* m, int mode, const orbfe_keypoint* keys_un,
                       const float* depth, const uint8_t* has_point, int n,
                       const orbfe_camera* cam, const float* rwc_ow, float th_depth,
                       int min_points, const float* scale_factors, int nlevels, int32_t* order,
                       int32_t* n_visited, uint8_t* create, float* xyz, float* max_dist,
                       float* min_dist, int32_t* n_total, int32_t* n_map);

/* Device-resident batch form: n_frames frames in slabs of kps_cap entries (d_n[f] valid), a pose
 * d_rwc_ow[12 f ..] per frame; the outputs are pitched alike (d_xyz: 3 kps_cap floats per frame)
 * and stay on the device, d_n_visited / d_n_total / d_n_map / d_status hold one int per frame
 * (d_status[f]: ORBFE_OK, ORBFE_ERR_CAPACITY or ORBFE_ERR_UNSUPPORTED).  scale_factors is a host
 * array.  Asynchronous on m's stream. */
int orbfe_close_points_batch_device(orbfe_matcher* m, int mode, int n_frames,
                                    const orbfe_keypoint* d_keys_un, const float* d_depth,
                                    const uint8_t* d_has_point, const int32_t* d_n, int kps_cap,
                                    const orbfe_camera* cam, const float* d_rwc_ow,
                                    float th_depth, int min_points, const float* scale_factors,
                                    int nlevels, int32_t* d_order, int32_t* d_n_visited,
                                    uint8_t* d_create, float* d_xyz, float* d_max_dist,
                                    float* d_min_dist, int32_t* d_n_total, int32_t* d_n_map,
                                    int32_t* d_status);

/* ---- bag of words (DBoW2, vendored in the reference as Thirdparty/DBoW2) ----------------- */

/* ORBVocabulary::loadFromTextFile (TemplatedVocabulary.h:1351-1436), called by System::System
 * on ORBvoc.txt: header "k L scoring weighting", one line per node "parent isLeaf d0..d31
 * weight".  The tree is kept in HBM of `device`.  Blank lines are skipped. */
orbfe_vocabulary* orbfe_vocabulary_load_text(const char* path, int device, int* status);
/* The same from node arrays: node 0 is the root (its entries are ignored); parent[i] < i
 * (anything else returns ORBFE_ERR_ARG); is_word flags the nodes that are words (word ids in
 * node order); desc n_nodes x 32.  A childless node that is no word sends its features to word
 * 0 with the node's weight, as the reference's Node() default does. */
orbfe_vocabulary* orbfe_vocabulary_create(int k, int L, int scoring, int weighting, int n_nodes,
                                          const int32_t* parent, const uint8_t* is_word,
                                          const uint8_t* desc, const double* weight, int device,
                                          int* status);
void orbfe_vocabulary_destroy(orbfe_vocabulary* v);
/* info[6] = {k, L, scoring, weighting, nodes, words}. */
int orbfe_vocabulary_info(const orbfe_vocabulary* v, int32_t* info);
int orbfe_vocabulary_set_stream(orbfe_vocabulary* v, void* hip_stream);

/* Frame::ComputeBoW / KeyFrame::ComputeBoW (Frame.cc:513-520) = TemplatedVocabulary::transform(
 * features, BowVector, FeatureVector, levelsup) (TemplatedVocabulary.h:1140-1196) over n
 * descriptors (n <= 4096).  BowVector: nw ascending word ids + values (double, normalised as the
 * vocabulary's scoring requires); FeatureVector: nn ascending node ids (level L - levelsup),
 * CSR offsets node_off[nn + 1] into feat (feature indices, ascending within a node).  Every
 * output array holds at least n entries (node_off n + 1).  Synchronous. */
int orbfe_bow_transform(orbfe_vocabulary* v, const uint8_t* desc, int n, int levelsup,
                        int32_t* word_ids, double* values, int32_t* nw, int32_t* node_ids,
                        int32_t* node_off, int32_t* feat, int32_t* nn);
/* Batched device form: frame f's descriptors at d_desc + f*cap*32 (d_n[f] rows, cap <= 4096);
 * outputs per frame at f*cap (node_off at f*(cap+1)), counts in d_nw[f] / d_nn[f].
 * Requires 0 <= d_n[f] <= cap for every frame: the kernels trust the count they read on the
 * device, and a larger one reads and writes past the frame's slot.  cap > 4096 returns
 * ORBFE_ERR_UNSUPPORTED.  Asynchronous on the vocabulary's stream (orbfe_vocabulary_set_stream). */
int orbfe_bow_transform_batch_device(orbfe_vocabulary* v, int nframes, const uint8_t* d_desc,
                                     const int32_t* d_n, int cap, int levelsup,
                                     int32_t* d_word_ids, double* d_values, int32_t* d_nw,
                                     int32_t* d_node_ids, int32_t* d_node_off, int32_t* d_feat,
                                     int32_t* d_nn);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)
 * (ORBmatcher.cc:159-291) with ORBmatcher(nnratio, check_ori) (Tracking.cc:1011 / 1621 use 0.7 /
 * 0.75, checkOri true).  Keyframe: n_kf descriptors, keypoint angles (mvKeysUn), kf_mp_ok[i] =
 * GetMapPointMatches()[i] != NULL && !isBad(), its FeatureVector (kf_nn nodes, CSR).  Frame: n_f
 * descriptors, angles (mvKeys) and FeatureVector.  matches[f] = the keyframe feature whose map
 * point lands in vpMapPointMatches[f], or -1; *nmatches as returned.  A common node holding more
 * than 256 frame features returns ORBFE_ERR_UNSUPPORTED (ORBvoc level-2 nodes hold ~10).  Each
 * FeatureVector must list a feature index under at most one node, as DBoW2 builds it
 * (FeatureVector.cpp:31-45); one that repeats an index returns ORBFE_ERR_ARG.  One kernel
 * launch per call (the common nodes' features gathered into pinned memory); the orientation
 * filter (ORBmatcher.cc:259-281) runs on the host, as in the reference. */
int orbfe_search_by_bow(orbfe_matcher* m, float nnratio, int check_ori, int n_kf,
                        const uint8_t* kf_desc, const float* kf_angle, const uint8_t* kf_mp_ok,
                        int kf_nn, const int32_t* kf_node_ids, const int32_t* kf_node_off,
                        const int32_t* kf_feat, int n_f, const uint8_t* f_desc,
                        const float* f_angle, int f_nn, const int32_t* f_node_ids,
                        const int32_t* f_node_off, const int32_t* f_feat, int32_t* matches,
                        int32_t* nmatches);

/* Batched device form of SearchByBoW for Tracking::Relocalization's candidate loop, which
 * matches the current frame against every relocalisation candidate keyframe with
 * ORBmatcher(0.75, true) (Tracking.cc:1621, 1636-1656): n_pairs (keyframe, frame) problems in
 * one call (n_pairs <= 65535).  Keyframes and frames are slots in the layout
 * orbfe_bow_transform_batch_device writes, with per-slot capacity kf_cap / f_cap: slot s holds
 * descriptors at d_*_desc + s*cap*32, angles (and the keyframe's map-point flags) at s*cap,
 * its FeatureVector's node ids and feature indices at s*cap, node offsets at s*(cap + 1) and
 * node count d_*_nn[s].  Pair p matches keyframe slot d_pair_kf[p] against frame slot
 * d_pair_f[p]; d_matches[p*f_cap + j] = the keyframe feature matched to frame feature j or -1
 * (all f_cap entries written), d_nmatches[p] = the returned count.  *d_status = 0, or
 * ORBFE_ERR_UNSUPPORTED (a common node over 256 frame features) / ORBFE_ERR_ARG (an offset or
 * index outside its slot; that node is skipped).  Asynchronous on the matcher's stream. */
int orbfe_search_by_bow_batch_device(orbfe_matcher* m, float nnratio, int check_ori, int n_pairs,
                                     const int32_t* d_pair_kf, const int32_t* d_pair_f,
                                     int kf_cap, const uint8_t* d_kf_desc,
                                     const float* d_kf_angle, const uint8_t* d_kf_mp_ok,
                                     const int32_t* d_kf_nn, const int32_t* d_kf_node_ids,
                                     const int32_t* d_kf_node_off, const int32_t* d_kf_feat,
                                     int f_cap, const uint8_t* d_f_desc, const float* d_f_angle,
                                     const int32_t* d_f_nn, const int32_t* d_f_node_ids,
                                     const int32_t* d_f_node_off, const int32_t* d_f_feat,
                                     int32_t* d_matches, int32_t* d_nmatches, int32_t* d_status);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
 * (ORBmatcher.cc:525-658), called by LoopClosing::ComputeSim3 with ORBmatcher(0.75, true) once
 * per loop candidate (LoopClosing.cc:266).  Keyframe k: nk descriptors, keypoint angles
 * (mvKeysUn), mp_okk[i] = GetMapPointMatches()[i] != NULL && !isBad() (561-565 for pKF1, 577-583
 * for pKF2) and its FeatureVector (nnk nodes, CSR), all caller-owned host arrays.  Differences
 * from orbfe_search_by_bow: the inner side needs a live map point too, a match needs
 * bestDist1 < TH_LOW (strict, 601), and the output is indexed by the KF1 feature:
 * matches12[i1] = the KF2 feature whose map point lands in vpMatches12[i1], or -1 (n1 entries);
 * *nmatches as returned.  A common node holding more than 256 KF2 features, or a rotation bin
 * beyond 30, returns ORBFE_ERR_UNSUPPORTED; a FeatureVector that repeats a
 * feature index returns ORBFE_ERR_ARG.  Synchronous. */
int orbfe_search_by_bow_keyframes(orbfe_matcher* m, float nnratio, int check_ori, int n1,
                                  const uint8_t* desc1, const float* angle1,
                                  const uint8_t* mp_ok1, int nn1, const int32_t* node_ids1,
                                  const int32_t* node_off1, const int32_t* feat1, int n2,
                                  const uint8_t* desc2, const float* angle2,
                                  const uint8_t* mp_ok2, int nn2, const int32_t* node_ids2,
                                  const int32_t* node_off2, const int32_t* feat2,
                                  int32_t* matches12, int32_t* nmatches);
/* Batched device form for ComputeSim3's candidate loop, which matches the current keyframe
 * against every loop candidate: n_pairs (pKF1, pKF2) problems in one call (n_pairs <= 65535).
 * Both sides are slots of one keyframe set in the layout orbfe_bow_transform_batch_device
 * writes, with per-slot capacity cap: slot s holds descriptors at d_desc + s*cap*32, angles and
 * map-point flags at s*cap, its FeatureVector's node ids and feature indices at s*cap, node
 * offsets at s*(cap + 1) and node count d_nn[s].  Pair p matches slot d_pair_kf1[p] (pKF1)
 * against slot d_pair_kf2[p]; d_matches12[p*cap + i1] = the KF2 feature matched to KF1 feature
 * i1 or -1 (all cap entries written), d_nmatches[p] = the returned count.  *d_status = 0, or
 * ORBFE_ERR_UNSUPPORTED / ORBFE_ERR_ARG (an offset or index outside its slot; that node is
 * skipped).  Asynchronous on the matcher's stream. */
int orbfe_search_by_bow_keyframes_batch_device(
    orbfe_matcher* m, float nnratio, int check_ori, int n_pairs, const int32_t* d_pair_kf1,
    const int32_t* d_pair_kf2, int cap, const uint8_t* d_desc, const float* d_angle,
    const uint8_t* d_mp_ok, const int32_t* d_nn, const int32_t* d_node_ids,
    const int32_t* d_node_off, const int32_t* d_feat, int32_t* d_matches12, int32_t* d_nmatches,
    int32_t* d_status);

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)
 * (ORBmatcher.cc:660-826, CheckDistEpipolarLine 140-157) with ORBmatcher(nnratio, check_ori):
 * LocalMapping::CreateNewMapPoints constructs ORBmatcher(0.6, false) and calls it once per
 * covisible neighbour (LocalMapping.cc:207-268).  nnratio is not read by this matcher.
 *   kf1, kf2      : mvKeysUn (x, y, octave, angle), mDescriptors and mvuRight (NULL: monocular)
 *                   of the two keyframes; kf2's scale_factors / nlevels are pKF2->mvScaleFactors
 *                   (the image bounds and grid constants are not read).
 *   has_mp1/2     : per feature, GetMapPoint(i) != NULL (705, 728).
 *   nn*, node_ids*, node_off*, feat* : mFeatVec of each keyframe as CSR (as orbfe_bow_transform
 *                   writes it).  Each must list a feature index under at most one node, as DBoW2
 *                   builds it; one that repeats an index returns ORBFE_ERR_ARG.
 *   f12           : the caller's F12 (LocalMapping::ComputeF12), 3 x 3 row-major.
 *   epipole       : ex, ey of 667-673 (include/orbfe_orbslam.hpp evaluates those lines).
 *   level_sigma2  : pKF2->mvLevelSigma2, kf2->nlevels floats.
 *   only_stereo   : bOnlyStereo.
 *   block_matched2: vbMatched2 (680) is read at 728 but never written in the reference, so the
 *                   literal source blocks nothing: 0 reproduces it (a keyframe-2 feature may be
 *                   matched by several keyframe-1 features).  1 builds the evident intent,
 *                   vbMatched2[bestIdx2] = true after 764, never released, not even when the
 *                   orientation filter later drops the match.
 * The winner of a keyframe-1 feature (no MapPoint; stereo under only_stereo) is, among the
 * keyframe-2 features of the same node that are unblocked, hold no MapPoint, are stereo under
 * only_stereo, lie at distance <= TH_LOW, are outside the epipole radius when both features are
 * monocular (746-752, float, strict <) and pass dsqr < 3.84 * mvLevelSigma2[octave] (a double
 * comparison; den == 0 fails), the one of smallest distance, last in node order on
 * ties.  The orientation filter (794-813) applies with check_ori.  matches12[i] (kf1->n entries)
 * = the keyframe-2 feature of keyframe-1 feature i or -1 (vMatches12; the pair list is its
 * compaction in ascending i), *nmatches as returned.  A common node holding more than 256
 * keyframe-2 features returns ORBFE_ERR_UNSUPPORTED, a keyframe-2 octave outside [0, nlevels)
 * ORBFE_ERR_ARG; that node / candidate is skipped and every other result is valid.  Angles
 * outside [0, 360) whose difference lands beyond bin 30 (where the reference writes outside
 * rotHist) return ORBFE_ERR_UNSUPPORTED and that match is dropped.  Synchronous. */
int orbfe_search_for_triangulation(orbfe_matcher* m, int check_ori, int block_matched2,
                                   int only_stereo, const orbfe_frame_view* kf1,
                                   const uint8_t* has_mp1, int nn1, const int32_t* node_ids1,
                                   const int32_t* node_off1, const int32_t* feat1,
                                   const orbfe_frame_view* kf2, const uint8_t* has_mp2, int nn2,
                                   const int32_t* node_ids2, const int32_t* node_off2,
                                   const int32_t* feat2, const float* f12, const float* epipole,
                                   const float* level_sigma2, int32_t* matches12,
                                   int32_t* nmatches);
/* Batched device form for CreateNewMapPoints' neighbour loop (LocalMapping.cc:215-268): n_pairs
 * (keyframe 1, keyframe 2) problems in one search launch (n_pairs <= 65535).  Keyframes are slots
 * of capacity cap in exactly the layout orbfe_bow_transform_batch_device reads and writes: slot
 * s holds descriptors at d_desc + s*cap*32, its FeatureVector's node ids and feature indices at
 * s*cap, node offsets at s*(cap + 1), node count d_nn[s]; and in addition keypoints at d_keys +
 * s*cap, mvuRight at d_u_right + s*cap (d_u_right NULL: monocular), map-point flags at d_has_mp
 * + s*cap and the feature count d_n[s].  Pair p matches slot d_pair_1[p] (pKF1) against slot
 * d_pair_2[p] (pKF2) with F12 = d_f12 + 9 p (row-major) and epipole d_epipole + 2 p.
 * scale_factors / level_sigma2 are HOST arrays of nlevels <= 16 floats shared by all keyframes
 * (read before the call returns).  d_matches12[p*cap + i] = the keyframe-2 feature of keyframe-1
 * feature i or -1 (all cap entries written), d_nmatches[p] = the returned count.  *d_status = 0,
 * or ORBFE_ERR_UNSUPPORTED (a common node over 256 keyframe-2 features) / ORBFE_ERR_ARG (an
 * offset or index outside its slot or count, a keyframe-2 octave outside [0, nlevels); that node
 * / feature is skipped).  Asynchronous on the matcher's stream. */
int orbfe_search_for_triangulation_batch_device(
    orbfe_matcher* m, int check_ori, int block_matched2, int only_stereo, int cap,
    const orbfe_keypoint* d_keys, const uint8_t* d_desc, const float* d_u_right,
    const uint8_t* d_has_mp, const int32_t* d_n, const int32_t* d_nn, const int32_t* d_node_ids,
    const int32_t* d_node_off, const int32_t* d_feat, int n_pairs, const int32_t* d_pair_1,
    const int32_t* d_pair_2, const float* d_f12, const float* d_epipole,
    const float* scale_factors, const float* level_sigma2, int nlevels, int32_t* d_matches12,
    int32_t* d_nmatches, int32_t* d_status);

/* ---- BoW scores and the keyframe database -------------------------------------------------- */

/* Which build of DBoW2's scoring loops orbfe_vocabulary_score* and the database queries
 * reproduce.  DBoW2 is compiled -O3 -march=native
 * (Thirdparty/DBoW2/CMakeLists.txt:4-5), so on an FMA host GCC contracts `score += vi * wi` of
 * the L2 and dot-product loops (ScoringObject.cpp:91, :290) into fma(vi, wi, score):
 * ORBFE_ARITH_X86_SIMD (the default) computes that, ORBFE_ARITH_SCALAR the uncontracted product
 * and sum.  L1, chi-square and Bhattacharyya have no product feeding an add and are the same in
 * both.  Applies to later calls. */
int orbfe_vocabulary_set_arithmetic(orbfe_vocabulary* v, int mode);

/* ORBVocabulary::score(v1, v2) (TemplatedVocabulary.h -> ScoringObject.cpp:23-311) with the
 * vocabulary's scoring: 0 L1 (:23-68), 1 L2 (:73-120), 2 chi-square (:125-170),
 * 4 Bhattacharyya (:226-266), 5 dot product (:271-311).  BowVectors are n ascending word ids +
 * values (as orbfe_bow_transform writes them; any values are accepted).  The common words' terms
 * are added to one double accumulator in ascending word order and the last step of each formula
 * is as written, so *score has the reference's bits (double sqrt and / are correctly rounded on
 * the device).  KL scoring (3, :175-221) returns ORBFE_ERR_UNSUPPORTED: it needs log, and the
 * device log is within 1 ulp, not correctly rounded.  Word ids that are not strictly ascending
 * return ORBFE_ERR_ARG.  Computed on the device; synchronous. */
int orbfe_vocabulary_score(orbfe_vocabulary* v, const int32_t* ids1, const double* vals1, int n1,
                           const int32_t* ids2, const double* vals2, int n2, double* score);
/* Batched device form, e.g. the minScore loop of LoopClosing::DetectLoop (LoopClosing.cc:125-139):
 * d_score[p] = score(slot d_pair_a[p], slot d_pair_b[p]) over slots in the layout
 * orbfe_bow_transform_batch_device writes (word ids / values at s*cap, d_nw[s]).  One wave per
 * pair; asynchronous on the vocabulary's stream. */
int orbfe_vocabulary_score_batch_device(orbfe_vocabulary* v, int n_pairs, const int32_t* d_pair_a,
                                        const int32_t* d_pair_b, int cap,
                                        const int32_t* d_word_ids, const double* d_values,
                                        const int32_t* d_nw, double* d_score);

/* The keyframe database, KeyFrameDatabase (KeyFrameDatabase.h:48-94): keyframes are slots of
 * device memory in the BoW-transform layout (word ids and values at s*cap, nw[s]); storage grows
 * by doubling inside orbfe_kfdb_add*, never inside a query, and never shrinks.  The device keeps
 * no inverted file: the order of the reference's walk over mvInvertedFile ("query words
 * ascending, each word's list in add order") is the sort key (first common word, add sequence).
 * A handle is not reentrant; the vocabulary must outlive it.  Queries run on the handle's own
 * stream (orbfe_kfdb_set_stream) with the vocabulary's scoring and arithmetic. */
typedef struct orbfe_kfdb orbfe_kfdb;

/* The per-keyframe query state the reference keeps on the KeyFrame (KeyFrame.h:166-171):
 * mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore.  The four
 * integers start at 0 (KeyFrame.cc:35, :64); the two scores are not initialised by the
 * reference: scores_set bit 0 / 1 tells whether loop_score / reloc_score was ever written (by a
 * query or orbfe_kfdb_set_scores). */
typedef struct orbfe_kfdb_state {
    uint64_t loop_query, reloc_query;
    int32_t  loop_words, reloc_words;
    float    loop_score, reloc_score;
    int32_t  scores_set;
    int32_t  reserved;
} orbfe_kfdb_state;

/* KeyFrameDatabase::KeyFrameDatabase (KeyFrameDatabase.cc:33-37).  cap <= 4096 words per
 * keyframe; slots_hint sizes the first allocation. */
orbfe_kfdb* orbfe_kfdb_create(orbfe_vocabulary* voc, int cap, int slots_hint, int* status);
void orbfe_kfdb_destroy(orbfe_kfdb* db);
int  orbfe_kfdb_set_stream(orbfe_kfdb* db, void* hip_stream);
/* Keyframes in the database. */
int  orbfe_kfdb_size(const orbfe_kfdb* db);

/* KeyFrameDatabase::add (KeyFrameDatabase.cc:115-121): a keyframe's BowVector (host arrays) into
 * a slot, returned in *slot; the most recently freed slot is reused first.  Each add takes the
 * next sequence number: add pushes the keyframe to the back of every word's list, so the order
 * inside every inverted list is add order, whatever the slot.  The slot's state is a new
 * KeyFrame's.  Word ids not strictly ascending, or one >= the vocabulary's word count (where the
 * reference indexes mvInvertedFile out of range), return ORBFE_ERR_ARG. */
int orbfe_kfdb_add(orbfe_kfdb* db, const int32_t* word_ids, const double* values, int nw,
                   int32_t* slot);
/* The same from device memory — one slot of a transform batch's output (d_word_ids + f*cap,
 * d_values + f*cap, d_nw + f): a device-to-device copy, validated on the device. */
int orbfe_kfdb_add_device(orbfe_kfdb* db, const int32_t* d_word_ids, const double* d_values,
                          const int32_t* d_nw, int32_t* slot);
/* KeyFrameDatabase::erase (KeyFrameDatabase.cc:123-142): frees the slot and removes it from
 * every covisibility list, so a neighbour entry never names a recycled slot.  A slot that is not
 * in use returns ORBFE_ERR_ARG. */
int orbfe_kfdb_erase(orbfe_kfdb* db, int slot);
/* KeyFrameDatabase::clear (KeyFrameDatabase.cc:144-148). */
int orbfe_kfdb_clear(orbfe_kfdb* db);
/* pKF->GetBestCovisibilityKeyFrames(10) (KeyFrame.cc:895-903) of the keyframe in `slot`, in its
 * order: n <= 10 slots.  A neighbour that is not in the database is passed as -1: it keeps its
 * place in the truncation and is skipped (no query can have touched it). */
int orbfe_kfdb_set_covisibility(orbfe_kfdb* db, int slot, int n, const int32_t* neigh_slots);
/* mLoopScore / mRelocScore of a keyframe loaded from a map archive (KeyFrame.cc:112-115). */
int orbfe_kfdb_set_scores(orbfe_kfdb* db, int slot, float loop_score, float reloc_score);
int orbfe_kfdb_get_state(orbfe_kfdb* db, int slot, orbfe_kfdb_state* state);

/* KeyFrameDatabase::DetectLoopCandidates(pKF, minScore) (KeyFrameDatabase.cc:151-272).
 * query_id = pKF->mnId, (word_ids, values, nw) = pKF->mBowVec, conn_slots = the slots of
 * pKF->GetConnectedKeyFrames() (:153), min_score = minScore.  cand receives vpLoopCandidates as
 * slots, in the reference's order; *n_cand their count (> cand_cap: ORBFE_ERR_CAPACITY and
 * nothing copied).  Every touched slot's state is updated as the reference updates the
 * KeyFrame, also on the early returns (:182, :216).  ORBFE_ERR_UNSUPPORTED with valid results:
 * the accumulation (:236) read a score that was never written, computed as 0.0f.
 * A query id equal to a slot's stored id (0 for a new keyframe) is reproduced literally
 * (DESIGN.md H19).  More than 4096 keyframes in lScoreAndMatch: ORBFE_ERR_CAPACITY with
 * *n_cand = that count (a limit of this implementation).  Either ORBFE_ERR_CAPACITY is returned
 * after the query ran: every touched slot's query id, word count and score are already
 * updated, as after a successful call, so a retry with a larger buffer must use a query id no
 * slot stores, or it takes the H19 path and answers differently.  One kernel launch; the host
 * waits on a done word in pinned memory. */
int orbfe_kfdb_detect_loop_candidates(orbfe_kfdb* db, uint64_t query_id, const int32_t* word_ids,
                                      const double* values, int nw, int n_conn,
                                      const int32_t* conn_slots, float min_score, int32_t* cand,
                                      int cand_cap, int32_t* n_cand);
/* KeyFrameDatabase::DetectRelocalizationCandidates(F) (KeyFrameDatabase.cc:274-389);
 * frame_id = F->mnId.  Otherwise as above (early returns :304, :335; the accumulation :353-356
 * tests mnRelocQuery only, so it may read the mRelocScore an earlier query left). */
int orbfe_kfdb_detect_relocalization_candidates(orbfe_kfdb* db, uint64_t frame_id,
                                                const int32_t* word_ids, const double* values,
                                                int nw, int32_t* cand, int cand_cap,
                                                int32_t* n_cand);
/* Device forms: the query vector (d_word_ids, d_values, *d_nw — e.g. one slot of a transform
 * batch's output) and the connected slots are read from device memory and the candidates are
 * left in d_cand (at most cand_cap written), ready to be the d_pair_kf of
 * orbfe_search_by_bow_batch_device or the d_pair_kf2 of
 * orbfe_search_by_bow_keyframes_batch_device; the count returns to the host in *n_cand, since
 * n_pairs of those calls is a host argument.  The host waits once, on the done word.  The
 * query vector is validated on the device before any state is touched: *d_nw outside
 * [0, cap of the database] (e.g. a transform batch with a larger cap) or word ids that are not
 * strictly ascending return ORBFE_ERR_ARG with *n_cand = 0, as the host forms do. */
int orbfe_kfdb_detect_loop_candidates_device(orbfe_kfdb* db, uint64_t query_id,
                                             const int32_t* d_word_ids, const double* d_values,
                                             const int32_t* d_nw, int n_conn,
                                             const int32_t* d_conn_slots, float min_score,
                                             int32_t* d_cand, int cand_cap, int32_t* n_cand);
int orbfe_kfdb_detect_relocalization_candidates_device(orbfe_kfdb* db, uint64_t frame_id,
                                                       const int32_t* d_word_ids,
                                                       const double* d_values,
                                                       const int32_t* d_nw, int32_t* d_cand,
                                                       int cand_cap, int32_t* n_cand);

/* ---- the local map: Tracking::UpdateLocalMap (Tracking.cc:1455-1599) ----------------------
 * A handle holds a device-resident mirror of the part of the map graph that
 * UpdateLocalKeyFrames (:1491-1599) and UpdateLocalPoints (:1465-1488) read.  Keyframes and map
 * points are dense slots handed out by the handle, in add order from 0.  There is no erase: the
 * reference never frees a KeyFrame or a MapPoint, it marks them bad; orbfe_map_clear mirrors
 * Tracking::Reset.  Device storage grows by doubling inside the mutators, never inside a query.
 * Per keyframe: the order key, the bad flag, mnTrackReferenceForFrame (the stamp), mvpMapPoints
 * as point slots or -1, GetBestCovisibilityKeyFrames(10), the children (kept sorted by order
 * key) and the parent.  Per point: the bad flag, mnTrackReferenceForFrame and the set of
 * observing keyframes.  The handle: mvpLocalKeyFrames and mpReferenceKF (-1 initially).
 *
 * Pointer order: the reference iterates map<KeyFrame*, int> and set<KeyFrame*>,
 * i.e. in the order of heap addresses.  Every keyframe carries a caller-supplied order_key and
 * "pointer order" is ascending key; with order_key = (uintptr_t)pKF the parity is exact for the
 * addresses the caller has.  Keys are distinct.
 * A handle is not reentrant.  The mutators are synchronous. */
typedef struct orbfe_map orbfe_map;

#define ORBFE_MAP_MAX_VOTED     4096   /* keyframes one call's frame points may vote for        */
#define ORBFE_MAP_MAX_KF_SLOTS  8192   /* mvpMapPoints of one keyframe                          */
#define ORBFE_MAP_KEYFRAMES     0      /* `kind` of orbfe_map_set_stamps / get_stamps           */
#define ORBFE_MAP_POINTS        1

orbfe_map* orbfe_map_create(int device, int keyframes_hint, int points_hint, int* status);
void orbfe_map_destroy(orbfe_map* m);
int  orbfe_map_set_stream(orbfe_map* m, void* hip_stream);
/* Tracking::Reset: no keyframes, no points, an empty list, reference keyframe -1.  Slots start
 * again from 0; the device storage is kept. */
int  orbfe_map_clear(orbfe_map* m);
int  orbfe_map_size(const orbfe_map* m, int32_t* n_keyframes, int32_t* n_points);

/* A new keyframe of n_slots <= 8192 keypoints: mp_slots[i] = the point held by keypoint i or -1
 * (NULL: all -1).  Not bad, stamp 0, no neighbours, children or parent.  A key already in the
 * map, n_slots out of range or a point slot that does not exist return ORBFE_ERR_ARG, as every
 * out-of-range slot does in every call below. */
int orbfe_map_add_keyframe(orbfe_map* m, uint64_t order_key, int n_slots, const int32_t* mp_slots,
                           int32_t* slot);
/* KeyFrame::AddMapPoint / EraseMapPointMatch / ReplaceMapPointMatch: entries [first, first + n)
 * of the keyframe's mvpMapPoints. */
int orbfe_map_set_keyframe_points(orbfe_map* m, int slot, int first, int n, const int32_t* mp_slots);
/* KeyFrame::SetBadFlag (mbBad). */
int orbfe_map_set_keyframe_bad(orbfe_map* m, int slot, int bad);
/* GetBestCovisibilityKeyFrames(10) of the keyframe, in its order: n <= 10 slots; -1 entries keep
 * their place and are skipped (the contract of orbfe_kfdb_set_covisibility).  Writes the ten
 * neighbours UpdateLocalKeyFrames reads and nothing else: the covisibility graph below
 * (weights, ordered list) is not touched, and the next call there that writes this keyframe's
 * ordered list overwrites the ten. */
int orbfe_map_set_covisibility(orbfe_map* m, int slot, int n, const int32_t* neigh_slots);
/* mspChildrens: the whole set, in any order; the handle sorts it by order key. */
int orbfe_map_set_children(orbfe_map* m, int slot, int n, const int32_t* child_slots);
/* mpParent, or -1. */
int orbfe_map_set_parent(orbfe_map* m, int slot, int parent);
/* n new points, slots *first_slot .. *first_slot + n - 1: not bad, stamp 0, no observations.
 * The pointer orbfe_map_local_points_device returned is invalid after this call. */
int orbfe_map_add_points(orbfe_map* m, int n, int32_t* first_slot);
/* MapPoint::SetBadFlag / mbBad of n points. */
int orbfe_map_set_points_bad(orbfe_map* m, int n, const int32_t* mp_slots, int bad);
/* MapPoint::AddObservation / EraseObservation, batched: point mp_slots[i] is (no longer) observed
 * by keyframe kf_slots[i].  Set semantics: a pair that is already (not) there is a no-op
 * (MapPoint.cc:170-171). */
int orbfe_map_add_observations(orbfe_map* m, int n, const int32_t* mp_slots, const int32_t* kf_slots);
int orbfe_map_erase_observations(orbfe_map* m, int n, const int32_t* mp_slots, const int32_t* kf_slots);
/* mnTrackReferenceForFrame of n keyframes (kind ORBFE_MAP_KEYFRAMES) or points (ORBFE_MAP_POINTS):
 * unsigned long, 0 for a new object, stored in the map archive (KeyFrame.cc:106, MapPoint.cc:80),
 * hence state with a getter and a setter.  The slots of one set call are distinct. */
int orbfe_map_set_stamps(orbfe_map* m, int kind, int n, const int32_t* slots, const uint64_t* stamps);
int orbfe_map_get_stamps(orbfe_map* m, int kind, int n, const int32_t* slots, uint64_t* stamps);
/* mvpLocalKeyFrames and mpReferenceKF assigned directly (Tracking.cc:789, :969-970): n <= 4104. */
int orbfe_map_set_local_keyframes(orbfe_map* m, int n, const int32_t* kf_slots, int ref_kf);
/* The list and the reference keyframe as the last query (or set) left them; host state.  *n > cap:
 * ORBFE_ERR_CAPACITY. */
int orbfe_map_get_local_keyframes(const orbfe_map* m, int32_t* kf_slots, int cap, int32_t* n,
                                  int32_t* ref_kf);

/* Tracking::UpdateLocalMap without the viewer call (:1458): UpdateLocalKeyFrames, then
 * UpdateLocalPoints, with mCurrentFrame.mnId = frame_id.  frame_mp: inout, n entries, the point
 * slot held by each frame keypoint or -1 (mCurrentFrame.mvpMapPoints); bad points are set to -1
 * (:1508).  local_kf receives mvpLocalKeyFrames in order (*n_local_kf entries), *ref_kf
 * mpReferenceKF, local_mp mvpLocalMapPoints in order (*n_local_mp entries).  Literal details:
 * bad keyframes are voted for but neither listed, stamped nor eligible as reference; an empty
 * vote returns early and the previous list and reference keyframe stay, UpdateLocalPoints still
 * runs over them (:1513); the neighbour loop stops while the list holds more than 80; the
 * parent is pushed without an isBad test and its break leaves the whole loop (:1588); a second
 * call with the same frame_id finds the stamps of the first.
 * A buffer that is too small returns ORBFE_ERR_CAPACITY with the true counts and copies nothing
 * into that buffer; the handle's state (stamps, list, reference keyframe, device point list) has
 * advanced as after a successful call, so a retry must not repeat the query: read the list with
 * orbfe_map_get_local_keyframes / orbfe_map_local_points_device.  More than 4096 voted keyframes
 * return ORBFE_ERR_CAPACITY with *n_local_kf = their number before any stamp, list or reference
 * keyframe is written; only the NULLing of bad points in frame_mp (idempotent) has happened.
 * Five kernel launches; the host waits once, on a done word in pinned memory. */
int orbfe_map_update_local(orbfe_map* m, uint64_t frame_id, int n, int32_t* frame_mp,
                           int32_t* local_kf, int kf_cap, int32_t* n_local_kf, int32_t* ref_kf,
                           int32_t* local_mp, int mp_cap, int32_t* n_local_mp);
/* The device form: d_frame_mp is the device array orbfe_search_by_projection_* /
 * orbfe_search_local_points_device update.  The point list stays in device memory
 * (orbfe_map_local_points_device); the keyframe list (host), *ref_kf and the counts come back
 * through pinned memory.  An entry of d_frame_mp outside [-1, points) is caught on the device:
 * ORBFE_ERR_ARG, nothing written but NULLed bad points. */
int orbfe_map_update_local_device(orbfe_map* m, uint64_t frame_id, int n, int32_t* d_frame_mp,
                                  int32_t* local_kf, int kf_cap, int32_t* n_local_kf,
                                  int32_t* ref_kf, int32_t* n_local_mp);
/* mvpLocalMapPoints of the last successful query as a device array of *n point slots, valid until
 * the next query or orbfe_map_add_points. */
int orbfe_map_local_points_device(const orbfe_map* m, const int32_t** d_list, int32_t* n);
/* The same list copied to the host (*n > cap: ORBFE_ERR_CAPACITY, nothing copied). */
int orbfe_map_get_local_points(orbfe_map* m, int32_t* mp_slots, int cap, int32_t* n);

/* Device arrays of map-point data: as `src` map-wide, indexed by point slot (mp_ids and bad are
 * not read: the handle has them); as `dst` contiguous, indexed by list position.  desc is 32
 * bytes per point and 16-byte aligned.  skip[i] != 0 <=> mnLastFrameSeen == the frame's id and
 * n_obs = Observations() are the caller's. */
typedef struct orbfe_map_point_arrays {
    float*   xyz;        /* n x 3 */
    float*   normal;     /* n x 3 */
    float*   min_dist;
    float*   max_dist;
    uint8_t* desc;       /* n x 32 */
    int32_t* n_obs;
    uint8_t* skip;
    int32_t* mp_ids;
    uint8_t* bad;
} orbfe_map_point_arrays;
/* The n points of d_list (device; e.g. orbfe_map_local_points_device) gathered in list order:
 * dst->mp_ids = the list, dst->bad = the handle's bad flags, the rest from src.  These are the
 * map-point inputs of orbfe_search_local_points_device.  An entry outside the map is written as
 * a bad point with id -1.  Asynchronous on the handle's stream. */
int orbfe_map_gather_points_device(orbfe_map* m, int n, const int32_t* d_list,
                                   const orbfe_map_point_arrays* src,
                                   const orbfe_map_point_arrays* dst);

/* ---- the covisibility graph: KeyFrame::UpdateConnections (KeyFrame.cc:1010-1100) ------------
 * Per keyframe of an orbfe_map, device-resident: mConnectedKeyFrameWeights as a row of
 * (slot, weight) in pointer order (ascending order key), mvpOrderedConnectedKeyFrames with
 * mvOrderedWeights, and mbFirstConnection (1 for a new keyframe).  The ordered list is state, not
 * a function of the weights: UpdateConnections leaves it thresholded at 15,
 * AddConnection re-sorts the whole weight map into it only when a weight changed.  A weight map
 * holds at most ORBFE_MAP_MAX_VOTED entries and a weight is at most ORBFE_MAP_MAX_KF_SLOTS.
 * Whenever a call below writes a keyframe's ordered list, its first ten entries (padded with -1)
 * become the neighbours UpdateLocalKeyFrames reads (orbfe_map_set_covisibility's data).  Device
 * storage grows inside these calls only.  All of them are synchronous; orbfe_map_clear resets
 * all of it.  The counting, the sorts, the upserts into the neighbours and their re-sorts run in
 * kernels; the host keeps row lengths and capacities only. */

/* UpdateConnections() on kf_slots[0 .. n) in that order, with the result of the reference's
 * sequential loop (n = 1: the online call; every keyframe: System.cc:188-191).  allow_parent[i]
 * is `mnId != 0` of keyframe i (NULL: all 1): with it and the first-connection flag set, the
 * parent becomes the front of the new ordered list, the keyframe joins the parent's children
 * (kept sorted by order key) and the flag is cleared.  parent_out[i] (or NULL) = the parent this
 * call assigned, else -1; n_ordered_out[i] (or NULL) = the length of the ordered list afterwards.
 * A keyframe whose points have no other observer is left exactly as it was (:1044).  Slots that
 * are out of range or not distinct: ORBFE_ERR_ARG.  A counter of more than 4096 keyframes, or a
 * neighbour's weight map that would pass 4096 entries: ORBFE_ERR_CAPACITY.  Either way nothing has
 * changed.  The batch is not cut into chunks: at most six kernel launches and five host waits
 * whatever n is (plus one of each when a parent was assigned). */
int orbfe_map_update_connections(orbfe_map* m, int n, const int32_t* kf_slots,
                                 const uint8_t* allow_parent, int32_t* parent_out,
                                 int32_t* n_ordered_out);
/* KeyFrame::AddConnection (:844-857): an absent key is inserted, a different weight overwritten,
 * both followed by UpdateBestCovisibles; an equal weight changes nothing.  0 <= weight <= 8192. */
int orbfe_map_add_connection(orbfe_map* m, int slot, int other, int weight);
/* KeyFrame::EraseConnection (:1295-1309): erases and re-sorts only if the key is present. */
int orbfe_map_erase_connection(orbfe_map* m, int slot, int other);
/* KeyFrame::UpdateBestCovisibles (:859-878): the ordered list becomes the whole weight map,
 * descending weight and, among equal weights, descending order key. */
int orbfe_map_update_best_covisibles(orbfe_map* m, int slot);
/* The connection part of KeyFrame::SetBadFlag (:1188-1189, :1198-1199): EraseConnection(slot) on
 * every key of the keyframe's weight map, then its own weight map and ordered list cleared. */
int orbfe_map_erase_keyframe_connections(orbfe_map* m, int slot);
/* Plain assignments, as a map archive holds them (KeyFrame.cc:400-443); nothing is re-sorted.
 * The weight map: n <= 4096 distinct keyframes in any order.  The ordered list with its weights:
 * n <= 4096 entries in the list's order (this one also writes the ten neighbours).  The flag. */
int orbfe_map_set_connections(orbfe_map* m, int slot, int n, const int32_t* kf_slots,
                              const int32_t* weights);
int orbfe_map_set_ordered_connections(orbfe_map* m, int slot, int n, const int32_t* kf_slots,
                                      const int32_t* weights);
int orbfe_map_set_first_connection(orbfe_map* m, int slot, int flag);
/* Read back from device memory.  The weight map in pointer order; the ordered list in its order;
 * weights may be NULL.  *n > cap: ORBFE_ERR_CAPACITY with nothing copied. */
int orbfe_map_get_connections(orbfe_map* m, int slot, int32_t* kf_slots, int32_t* weights, int cap,
                              int32_t* n);
int orbfe_map_get_ordered_connections(orbfe_map* m, int slot, int32_t* kf_slots, int32_t* weights,
                                      int cap, int32_t* n);
/* mpParent (or -1), mbFirstConnection and mspChildrens in pointer order; parent and
 * first_connection may be NULL. */
int orbfe_map_get_spanning_tree(orbfe_map* m, int slot, int32_t* parent, int32_t* first_connection,
                                int32_t* child_slots, int cap, int32_t* n_children);

/* ---- culling: LocalMapping::MapPointCulling (LocalMapping.cc:170-205) and what it reads -------
 * More state of an orbfe_map, all of it plain state with a setter and a getter and
 * reset by orbfe_map_clear.  Per keyframe keypoint: mvKeysUn[i].octave, whether mvuRight[i] >= 0,
 * mvDepth[i]; per keyframe mThDepth.  Per observation: the feature index mObservations[pKF], or -1
 * for an observation added without one.  Per point: nObs (state, not the size of the observation
 * set: MapPoint::SetBadFlag clears the set and leaves nObs), mnFound and mnVisible (1 for a new
 * point), mnFirstKFid (0).  orbfe_map_add_observations records the index -1 and adds 1 to nObs;
 * orbfe_map_erase_observations subtracts what the stored index says (1 for -1) and never sets a
 * point bad.  All calls are synchronous. */

#define ORBFE_MAP_FOUND    0   /* `kind` of orbfe_map_increase_counters */
#define ORBFE_MAP_VISIBLE  1

/* The keypoints of a keyframe: n must equal its slot count.  octaves in [0, 127] (NULL: all 0),
 * mvu_right (NULL: all -1; only `>= 0` is kept), depth (NULL: all -1).  A keyframe that never had
 * the call reads as octave 0, no right coordinate, depth -1, th_depth 0.  An octave out of range:
 * ORBFE_ERR_ARG with nothing written. */
int orbfe_map_set_keyframe_features(orbfe_map* m, int slot, int n, const int32_t* octaves,
                                    const float* mvu_right, const float* depth, float th_depth);
/* octaves, has_right, depth and th_depth may be NULL; *n > cap: ORBFE_ERR_CAPACITY. */
int orbfe_map_get_keyframe_features(orbfe_map* m, int slot, int cap, int32_t* octaves,
                                    uint8_t* has_right, float* depth, float* th_depth, int32_t* n);
/* MapPoint::AddObservation(pKF, idx) (MapPoint.cc:339-350), batched: a pair already present is a
 * no-op (its index stays); else the index is stored and nObs grows by 2 if the keyframe's right
 * flag at idx is set, else by 1.  idx outside the keyframe's slots: ORBFE_ERR_ARG. */
int orbfe_map_add_observations_idx(orbfe_map* m, int n, const int32_t* mp_slots,
                                   const int32_t* kf_slots, const int32_t* idx);
/* MapPoint::EraseObservation(pKF) (:352-378): an absent pair is a no-op; else nObs goes down by 2
 * or 1 by the right flag at the stored index, the pair is erased and, if nObs <= 2, the point's
 * SetBadFlag runs (*went_bad = 1; may be NULL).  mpRefKF follows (:367-368; see the
 * refresh section below). */
int orbfe_map_erase_observation(orbfe_map* m, int mp_slot, int kf_slot, int32_t* went_bad);
/* MapPoint::SetBadFlag (:392-409) of n points: the bad flag set, the observation row cleared (nObs
 * untouched) and EraseMapPointMatch(idx) on every former observer: entry idx of that keyframe's
 * mvpMapPoints becomes -1 whatever it held.  A listed point with an observation of index -1:
 * ORBFE_ERR_ARG before anything changes.  One launch, a wave per point. */
int orbfe_map_set_point_bad_flag(orbfe_map* m, int n, const int32_t* mp_slots);
/* nObs, mnFound, mnVisible, mnFirstKFid of n points (distinct slots for the setter); an array
 * that is NULL is left alone / not read back. */
int orbfe_map_set_point_counters(orbfe_map* m, int n, const int32_t* mp_slots, const int32_t* n_obs,
                                 const int32_t* found, const int32_t* visible,
                                 const int64_t* first_kf_id);
int orbfe_map_get_point_counters(orbfe_map* m, int n, const int32_t* mp_slots, int32_t* n_obs,
                                 int32_t* found, int32_t* visible, int64_t* first_kf_id);
/* MapPoint::IncreaseFound / IncreaseVisible(amounts[i]) (NULL: 1) of n points; a repeated slot
 * adds up. */
int orbfe_map_increase_counters(orbfe_map* m, int kind, int n, const int32_t* mp_slots,
                                const int32_t* amounts);
/* The same by 1 from a device array of n point slots (e.g. the d_frame_mp of
 * orbfe_search_local_points_device) and an optional device byte mask (e.g. its in_view): entries
 * of -1 and entries whose mask byte is 0 are skipped.  An entry outside [-1, points) is caught on
 * the device: ORBFE_ERR_ARG with nothing added. */
int orbfe_map_increase_counters_device(orbfe_map* m, int kind, int n, const int32_t* d_mp_slots,
                                       const uint8_t* d_mask);
/* LocalMapping::MapPointCulling.  list: inout, mlpRecentAddedMapPoints as n_in point slots (a point
 * may repeat: the later occurrence sees the bad flag the earlier one set); afterwards its first
 * *n_out entries are the list that remains, in order.  culled (n_in entries): the *n_culled points
 * whose SetBadFlag ran, in order.  In the reference's order: bad -> dropped;
 * (float)mnFound / mnVisible < 0.25f -> SetBadFlag and dropped (mnVisible 0 gives inf or NaN: kept);
 * (int)current - (int)mnFirstKFid >= 2 and nObs <= (monocular ? 2 : 3) -> SetBadFlag and dropped;
 * difference >= 3 -> dropped; else kept.  current_kf_id or the mnFirstKFid of a listed point that is
 * not bad outside [0, 2^31), or a culled point with an observation of index -1: ORBFE_ERR_ARG with
 * nothing changed.  Two launches (deciding in one workgroup; a wave per culled point) and two host
 * waits. */
int orbfe_map_cull_points(orbfe_map* m, int64_t current_kf_id, int monocular, int32_t* list, int n_in,
                          int32_t* n_out, int32_t* culled, int32_t* n_culled);
/* KeyFrame::TrackedMapPoints(min_obs) (KeyFrame.cc:971-996): the keyframe's entries that are not
 * NULL, not bad and, when min_obs > 0, have nObs >= min_obs. */
int orbfe_map_tracked_map_points(orbfe_map* m, int slot, int min_obs, int32_t* n);
/* Read back from device memory: mvpMapPoints of a keyframe; the observation row of a point (in
 * ascending keyframe slot) with its indices (idx may be NULL); mbBad of n keyframes or points
 * (`kind` as in orbfe_map_get_stamps).  *n > cap: ORBFE_ERR_CAPACITY. */
int orbfe_map_get_keyframe_points(orbfe_map* m, int slot, int32_t* mp_slots, int cap, int32_t* n);
int orbfe_map_get_observations(orbfe_map* m, int mp_slot, int32_t* kf_slots, int32_t* idx, int cap,
                               int32_t* n);
int orbfe_map_get_bad_flags(orbfe_map* m, int kind, int n, const int32_t* slots, uint8_t* bad);

/* ---- culling: KeyFrame::SetBadFlag complete (KeyFrame.cc:1174-1287) and
 * LocalMapping::KeyFrameCulling (LocalMapping.cc:632-698) --------------------------------------
 * Per keyframe, more plain state: mbNotErase and mbToBeErased (KeyFrame.cc:1152-1186), both 0 for
 * a new keyframe.  mTcp, Map::EraseKeyFrame and KeyFrameDatabase::erase stay with the caller
 * (orbfe_kfdb_erase); mpRefKF of a point follows each EraseObservation (the refresh section below). */

#define ORBFE_MAP_BAD_NOTHING   0   /* *what of a SetBadFlag: mnId == 0, nothing changed          */
#define ORBFE_MAP_BAD_DEFERRED  1   /* mbNotErase: mbToBeErased set, nothing else                 */
#define ORBFE_MAP_BAD_DONE      2
#define ORBFE_MAP_CULL_KEPT     0   /* result[] of orbfe_map_cull_keyframes                       */
#define ORBFE_MAP_CULL_CULLED   1
#define ORBFE_MAP_CULL_DEFERRED 2
#define ORBFE_MAP_MAX_CULL_LIST 4096

int orbfe_map_set_not_erase(orbfe_map* m, int slot, int flag);
int orbfe_map_get_erase_flags(orbfe_map* m, int slot, int32_t* not_erase, int32_t* to_be_erased);
/* KeyFrame::SetBadFlag.  is_first (`mnId == 0`): nothing changes.  mbNotErase: mbToBeErased is set
 * and nothing else.  Otherwise, in the reference's order: the connection part
 * (orbfe_map_erase_keyframe_connections); EraseObservation(this) on every non-NULL entry of
 * mvpMapPoints (the keyframe leaves the point's row, nObs goes down by 2 or 1 by the right flag at
 * the observation's index, a point left with nObs <= 2 has its SetBadFlag run; a point held at two
 * indices is erased once, a point that does not list the keyframe is untouched, the keyframe's own
 * entries stay); the spanning tree (:1201-1280): candidates are the parent; per round, over the
 * children that are not bad in pointer order and each one's ordered list as it stands, the first
 * largest GetWeight (read from the weight map, 0 when absent) towards a candidate changes that
 * child's parent, makes it a candidate and removes it from mspChildrens; the children left over,
 * bad ones included, go to the parent if there is one (mspChildrens is not cleared then) and keep
 * this keyframe otherwise; EraseChild on the parent; mbBad.
 * bad_points: the points whose SetBadFlag ran, in slot order of the entries; pairs: (child, new
 * parent) as 2 x *n_pairs ints in the order of the ChangeParent calls.  A buffer that is too
 * small: ORBFE_ERR_CAPACITY with the true counts, the state changed as after a successful call.  A
 * point that would go bad while another observer of it has index -1: ORBFE_ERR_ARG before anything
 * changes.  Three launches of a wave per held point (marking, checking, applying), the
 * connection part's launches, one workgroup for the lists and the tournament; the host waits
 * after the check, inside the connection part and on the done word. */
int orbfe_map_set_keyframe_bad_flag(orbfe_map* m, int slot, int is_first, int32_t* what,
                                    int32_t* bad_points, int bad_cap, int32_t* n_bad,
                                    int32_t* pairs, int pair_cap, int32_t* n_pairs);
/* KeyFrame::SetErase (:1158-1172): clears mbNotErase unless has_loop_edges, then runs SetBadFlag as
 * above if mbToBeErased. */
int orbfe_map_set_erase(orbfe_map* m, int slot, int has_loop_edges, int is_first, int32_t* what,
                        int32_t* bad_points, int bad_cap, int32_t* n_bad, int32_t* pairs,
                        int pair_cap, int32_t* n_pairs);
/* LocalMapping::KeyFrameCulling with the result of the reference's sequential loop.  The list:
 * kf_slots[0 .. n), or with kf_slots NULL the ordered covisibility list of current_slot as it
 * stands (copied before anything is culled); *n_listed its length, result[i] one of
 * ORBFE_MAP_CULL_*.  first_kf_slot (`mnId == 0`, or -1) is skipped.  Per keyframe: mvpMapPoints as
 * a vector (a point held twice counts twice), NULL and bad skipped; unless monocular, entries with
 * mvDepth > mThDepth or mvDepth < 0 skipped (float compares: NaN and -0 count); nMPs counts the
 * rest; a point with nObs > 3 is redundant when three observers other than the keyframe have an
 * octave (at their index) <= the entry's octave + 1; culled when nRedundant > 0.9 * nMPs, by the
 * full SetBadFlag above (a mbNotErase keyframe is deferred).  One launch decides every listed
 * keyframe (a workgroup each); the first that culls, in list order, has seen an unchanged map: its
 * SetBadFlag is applied and only the keyframes after it decide again: culled + 1 decide launches
 * and host waits, plus what each SetBadFlag costs.  bad_points and pairs as above, concatenated
 * in the order of the culls.  More than 4,096 listed keyframes or *n_listed > result_cap:
 * ORBFE_ERR_CAPACITY with nothing changed.  While any observation of the map has index -1:
 * ORBFE_ERR_ARG with nothing changed (an observer's octave could not be read). */
int orbfe_map_cull_keyframes(orbfe_map* m, int current_slot, int n, const int32_t* kf_slots,
                             int first_kf_slot, int monocular, int32_t* result, int result_cap,
                             int32_t* n_listed, int32_t* bad_points, int bad_cap, int32_t* n_bad,
                             int32_t* pairs, int pair_cap, int32_t* n_pairs);

/* ---- MapPoint refresh: UpdateNormalAndDepth (MapPoint.cc:571-619), ComputeDistinctiveDescriptors
 * (:483-548) and the map-point loop of LocalMapping::ProcessNewKeyFrame (LocalMapping.cc:140-161) --
 * More plain state of an orbfe_map, each item with a setter and a getter, reset by
 * orbfe_map_clear, carried over by growth, and made by the first call that needs it.  Per map:
 * mvScaleFactors.  Per keyframe: GetCameraCenter() as three floats, (0, 0, 0) until set.  Per
 * keyframe keypoint: its row of mDescriptors, 32 bytes, with a per-keyframe "set" flag.  Per point:
 * mpRefKF as a keyframe slot or -1 (the default).
 * mpRefKF follows every erase as MapPoint.cc:367-368 has it: when the observation of keyframe k is
 * erased and the point's reference is k, the reference becomes mObservations.begin()->first, the
 * remaining observer with the lowest order key, before the `nObs <= 2` decision (a point that goes
 * bad on that erase has the new reference; SetBadFlag leaves it).  Where nothing remains the
 * reference dereferences begin() of an empty map; the mirror stores -1.  This holds for
 * orbfe_map_erase_observation, orbfe_map_erase_observations and the erases of a keyframe's
 * SetBadFlag, from the first call that touches mpRefKF on.  From then on the two host erase calls
 * read the references of the listed points back first (one more host wait per call) and write
 * the changed ones after the rows (one more launch and wait, only when one changed). */

#define ORBFE_MAP_REFRESH_NORMAL_DEPTH 1      /* bits of `what` and of result[]                    */
#define ORBFE_MAP_REFRESH_DESCRIPTOR   2
#define ORBFE_MAP_REFRESH_UNSUPPORTED  4      /* result[] only: the entry's normal and distances   */
                                              /* were left alone (see ORBFE_ERR_UNSUPPORTED below) */
#define ORBFE_MAP_MAX_REFRESH_OBS      1024   /* observers of one refreshed point                  */

/* mvScaleFactors: 1 <= nlevels <= 128.  The getter: *nlevels = 0 while never set; > cap:
 * ORBFE_ERR_CAPACITY. */
int orbfe_map_set_scale_factors(orbfe_map* m, int nlevels, const float* scale);
int orbfe_map_get_scale_factors(const orbfe_map* m, float* scale, int cap, int32_t* nlevels);
/* GetCameraCenter() of n keyframes: ow holds 3 n floats. */
int orbfe_map_set_keyframe_centers(orbfe_map* m, int n, const int32_t* kf_slots, const float* ow);
int orbfe_map_get_keyframe_centers(orbfe_map* m, int n, const int32_t* kf_slots, float* ow);
/* mDescriptors of a keyframe, n x 32 bytes; n must equal its slot count.  The device form copies
 * from a device pointer (e.g. a row of the batch extraction's slab) on the handle's stream.  The
 * getter: *is_set (may be NULL) = whether a set call has run; rows never set read zero; *n > cap:
 * ORBFE_ERR_CAPACITY. */
int orbfe_map_set_keyframe_descriptors(orbfe_map* m, int slot, int n, const uint8_t* desc);
int orbfe_map_set_keyframe_descriptors_device(orbfe_map* m, int slot, int n, const uint8_t* d_desc);
int orbfe_map_get_keyframe_descriptors(orbfe_map* m, int slot, int cap, uint8_t* desc, int32_t* n,
                                       int32_t* is_set);
/* mpRefKF of n points (distinct slots for the setter): a keyframe slot or -1. */
int orbfe_map_set_point_ref_keyframes(orbfe_map* m, int n, const int32_t* mp_slots,
                                      const int32_t* kf_slots);
int orbfe_map_get_point_ref_keyframes(orbfe_map* m, int n, const int32_t* mp_slots, int32_t* kf_slots);

/* UpdateNormalAndDepth (what & 1) and ComputeDistinctiveDescriptors (what & 2) of the n listed
 * points.  `arrays` is the map-wide device struct orbfe_map_gather_points_device takes as src: xyz
 * is read; normal, min_dist, max_dist and desc are written in place at the point's slot; the other
 * members are ignored and may be NULL.  Entries of -1 and bad points are skipped (mbBad returns
 * first in both functions); a point listed twice gets the same bytes twice.  result (may be NULL):
 * per entry the bits of what was written, and ORBFE_MAP_REFRESH_UNSUPPORTED.
 * Both functions walk the observations in pointer order (ascending order key, H26); that order
 * picks the first descriptor on a median tie and is the order of the normal's float sum.
 * The descriptor: observers whose keyframe is bad are left out (:506); none left: desc stays; the
 * rest as orbfe_distinctive_descriptors, observer j's descriptor being row idx_j of its keyframe.
 * The normal and the distances, literally: every observer counts, bad keyframes too;
 *   d = Pos - Ow_i (float); a = (float)(1.0 / sqrt(sum (double)d_k d_k)); acc_k = acc_k + d_k a
 * (product rounded before the add), sequentially in pointer order; pRefKF == NULL leaves all three
 * outputs alone (:600), the normal too; else, pRefKF not tested for isBad,
 *   dist = (float)sqrt(..) of Pos - Ow_ref; level = pRefKF's octave at observations[pRefKF]
 * (operator[] on the copy: index 0 when pRefKF is not an observer; n is not affected);
 *   max = dist scale[level]; min = max / scale[nlevels - 1]; normal_k = acc_k (float)(1.0 / n).
 * ORBFE_ERR_ARG with nothing written: a list entry outside [-1, points); a live listed point with
 * an observation of index -1; what & 1 without a scale table; what & 2 where a non-bad observer's
 * keyframe has no descriptors set.  ORBFE_ERR_CAPACITY with nothing written: a live listed point
 * with more than 1,024 observers (the reference puts float Distances[N][N] on the stack).
 * ORBFE_ERR_UNSUPPORTED: a point whose reference octave is >= nlevels, or whose reference keyframe
 * has no keypoint at the index read (the reference reads out of range): that point's normal and
 * distances stay and its result carries ORBFE_MAP_REFRESH_UNSUPPORTED; everything else is written.
 * Two launches of a wave per entry: a check launch that writes nothing but the error word, an
 * apply launch that returns at once when that word holds a refusal.  The host waits once, on the
 * done word; the host form's masks come back through pinned memory.  The device forms read the
 * list, and write d_result, in device memory. */
int orbfe_map_refresh_points(orbfe_map* m, int what, int n, const int32_t* mp_slots,
                             const orbfe_map_point_arrays* arrays, uint8_t* result);
int orbfe_map_refresh_points_device(orbfe_map* m, int what, int n, const int32_t* d_list,
                                    const orbfe_map_point_arrays* arrays, uint8_t* d_result);
/* The same over the keyframe's mvpMapPoints where it lies (the loop of LocalMapping.cc:518-530);
 * nothing is uploaded.  *n_refreshed (may be NULL): the entries that hold a point that is not bad. */
int orbfe_map_refresh_keyframe_points(orbfe_map* m, int kf_slot, int what,
                                      const orbfe_map_point_arrays* arrays, int32_t* n_refreshed);
/* The map-point loop of ProcessNewKeyFrame over index i of the keyframe's mvpMapPoints: NULL and
 * bad entries are skipped; a point the keyframe does not observe yet gets AddObservation(kf, i)
 * (nObs rises by 2 or 1 by the right flag) and both refreshes; any other is appended to `recent`
 * (mlpRecentAddedMapPoints), in index order.  A point held at two indices is added at the lower
 * one and listed in recent at the higher one.  recent_cap too small: ORBFE_ERR_CAPACITY with the
 * true count and nothing changed.  ComputeBoW, UpdateConnections and Map::AddKeyFrame stay the
 * separate calls they are.  What the refresh would refuse (see orbfe_map_refresh_points; also a
 * keyframe whose descriptors were never set, bad or not, while it has a point to add) is found
 * first: ORBFE_ERR_ARG or ORBFE_ERR_CAPACITY with nothing changed.  Four steps: one classifying
 * launch (a thread per slot; one wait on the done word), one check launch over what is new (one
 * wait), orbfe_map_add_observations_idx of it (two launches, two waits), then
 * orbfe_map_refresh_points of the same (two launches, one wait), which can only return
 * ORBFE_OK or ORBFE_ERR_UNSUPPORTED by then. */
int orbfe_map_process_new_keyframe(orbfe_map* m, int kf_slot, const orbfe_map_point_arrays* arrays,
                                   int32_t* recent, int recent_cap, int32_t* n_recent);

/* ---- map-archive records of the extractor outputs (device side) ---------------------------
 * The bodies the reference's Boost map archive stores for the extractor's outputs, written
 * from / read into HBM (MapPoint.h:196-247; KeyFrame::serialize KeyFrame.cc:133-134 / 354-355
 * stores mvKeys, mvKeysUn and mDescriptors, MapPoint::serialize MapPoint.cc:121 / 194 stores
 * mDescriptor).  Keypoint record (serialize(Archive&, cv::KeyPoint&), MapPoint.h:196-209):
 * angle, class_id, octave, response, response, pt.x, pt.y — 28 bytes, size not stored (a
 * loaded keypoint has size 0).  cv::Mat record (save / load, MapPoint.h:215-247): cols i32,
 * rows i32, elemSize u64, type u64, raw bytes; descriptors are rows x 32 CV_8UC1.  Boost's
 * own framing (class-info preamble, collection counts) is the archive writer's.  All entry
 * points are asynchronous on hip_stream (NULL = the null stream) of the current device and take
 * at most 65535 frames / Mats per call. */

/* Bytes of one cv::Mat record: 24 + rows * cols * elem_size (-1 on negative arguments). */
int64_t orbfe_archive_mat_bytes(int rows, int cols, int elem_size);
/* Frame f's min(d_n[f], cap) keypoints (d_keys + f*keys_pitch, orbfe_keypoint units) as
 * consecutive 28-byte records at d_out + f*out_pitch (bytes; a multiple of 4, >= 28*cap). */
int orbfe_archive_write_keypoints_device(int n_frames, const orbfe_keypoint* d_keys,
                                         size_t keys_pitch, const int32_t* d_n, int cap,
                                         uint8_t* d_out, size_t out_pitch, void* hip_stream);
/* The inverse: min(d_n[f], cap) records -> keypoints (size 0, response = the second value). */
int orbfe_archive_read_keypoints_device(int n_frames, const uint8_t* d_in, size_t in_pitch,
                                        const int32_t* d_n, int cap, orbfe_keypoint* d_keys,
                                        size_t keys_pitch, void* hip_stream);
/* Mat k's descriptors (d_desc + k*desc_pitch, rows = d_rows[k], or rows_fixed when d_rows is
 * NULL — 1 for MapPoint::mDescriptor — clipped to cap) as one rows x 32 CV_8UC1 record at
 * d_out + k*out_pitch; d_len[k] (may be NULL) = its bytes.  Pitches are multiples of 8,
 * out_pitch >= orbfe_archive_mat_bytes(cap, 32, 1). */
int orbfe_archive_write_descriptors_device(int n_mats, const uint8_t* d_desc, size_t desc_pitch,
                                           const int32_t* d_rows, int rows_fixed, int cap,
                                           uint8_t* d_out, size_t out_pitch, int64_t* d_len,
                                           void* hip_stream);
/* Reads n_mats descriptor records (d_in + k*in_pitch) into d_desc + k*desc_pitch; d_rows[k]
 * (may be NULL) = rows, or -1 for a record whose header is not (32, rows <= cap, 1, CV_8UC1),
 * which sets *d_status = ORBFE_ERR_ARG (0 otherwise). */
int orbfe_archive_read_descriptors_device(int n_mats, const uint8_t* d_in, size_t in_pitch,
                                          int cap, uint8_t* d_desc, size_t desc_pitch,
                                          int32_t* d_rows, int32_t* d_status, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* ORBFE_H */
