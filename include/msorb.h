/* msorb — MI355X-native ORB front-end for MS-SLAM: C ABI of libmsorb.so.
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes plain
 * pointers and sizes, never throws, never allocates across the boundary, and returns MSORB_OK (0)
 * or a negative MSORB_E_* code (msorb_last_error() gives the thread-local detail string).
 * Each function names the reference interface it replaces (paths are into fishmarch/MS-SLAM).
 *
 * The kernels are hand-written HIP for gfx950; there is NO CPU fallback: on a machine without a
 * usable GPU every compute entry returns MSORB_E_NO_DEVICE.
 */
#ifndef MSORB_H
#define MSORB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSORB_OK 0
#define MSORB_E_INVALID -1    /* bad argument */
#define MSORB_E_NO_DEVICE -2  /* no HIP device / HIP runtime error at init */
#define MSORB_E_HIP -3        /* HIP runtime error during the call: outputs and in/out arrays (frame_mp, cur_mp, matched, ...)
                                 are unspecified — the claim-replaying searches may have applied the accepts of earlier rounds */
#define MSORB_E_CAPACITY -4   /* caller-provided buffer too small */
#define MSORB_E_GEOMETRY -5   /* image too small for the reference's cell arithmetic (it would divide by zero) */
#define MSORB_E_EMPTY -6      /* empty input image: ORBextractor::operator() returns -1 (ORBextractor.cc:1090-1091) */

#define MSORB_MAX_LEVELS 16
#define MSORB_DESC_BYTES 32

/* Same 28-byte layout as cv::KeyPoint (pt.x, pt.y, size, angle, response, octave, class_id). */
typedef struct msorb_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} msorb_keypoint;

const char* msorb_last_error(void);
int msorb_device_count(void);
/* Free / total memory of a device in bytes (hipMemGetInfo): what a long-running integration watches to see that the library's
 * resident state — extractor handles, matcher frames, the KeyFrame store — stays bounded (tests/soak_main.cc).  Since ABI 6000. */
int msorb_device_memory(int device, size_t* free_bytes, size_t* total_bytes);

/* ABI version of the library that was loaded: MSORB_ABI_VERSION of the header it was BUILT from.  major * 1000 + minor; a new
 * minor only appends entry points (or appends `_ex` forms with more parameters), a new major changes or removes one.  The host
 * classes (host/ORBextractor.cc, host/ORBmatcher_device.h) and the Python mirror compare msorb_abi_version() with the header
 * they were compiled against and refuse a library with another major or an older minor (msorb_abi_compatible). */
#define MSORB_ABI_VERSION 6002
int msorb_abi_version(void);
/* 1 if a caller compiled against `header_version` may use this library (same major, library minor >= header minor). */
int msorb_abi_compatible(int header_version);

/* Process-wide fatal-error callback of the host layer.  The reference's ORBextractor / ORBmatcher cannot fail and their callers
 * (Tracking.cc, LocalMapping.cc, LoopClosing.cc) have no handler around them, so the drop-in classes end the process on a lost
 * GPU the way the reference ends it on its own fatal conditions (message + exit(-1), System.cc:117-120).  An embedding
 * application registers a callback to get control FIRST (flush the map / atlas, log, raise its own flag): the host classes call
 * msorb_notify_fatal(code, what) before their default action (MSORB_THROW=1: throw std::runtime_error, else message + exit(-1));
 * the callback may itself not return (exit, longjmp, throw through C++ frames).  fn == NULL unregisters.  Thread safe; the
 * callback runs on the thread that hit the error.  The C entry points themselves never call it: they return MSORB_E_*. */
typedef void (*msorb_fatal_fn)(int code, const char* what, void* user);
void msorb_set_fatal_callback(msorb_fatal_fn fn, void* user);
void msorb_notify_fatal(int code, const char* what);

/* ------------------------------------------------------------------------------------------------
 * Host-memory admission — images the per-frame entries read IN PLACE.  Since ABI 6002.
 *
 * The reference reads the caller's cv::Mat where it lies (ORBextractor.cc:1190).  Here a per-frame entry (msorb_extract,
 * msorb_extract_pair, msorb_extract_stereo and the frame / tracking entries on it, msorb_extract_stereo_split) looks each image's
 * byte range [image, image + (rows-1)*stride + cols) up in a process-wide table of pinned host memory.  A range wholly inside ONE
 * entry is read by the upload kernel straight from the caller's memory: no staging copy, and both eyes of a stereo frame in one
 * launch.  Anything else — pageable memory, a range that overhangs its entry by one byte, an entry that has left the table — takes
 * the staged path, with identical results.  The decision is per image.  The table is the only source of host addresses a kernel
 * dereferences: nothing is remembered by raw pointer, so memory that was freed and handed out again never looks pinned.
 * An entry is in use from a call's lookup until that call has synchronised its stream: msorb_host_free / msorb_host_unregister
 * of an entry in use return MSORB_E_INVALID and free nothing.  Thread safe; usable before any handle exists; without a HIP
 * device the alloc / register entries return MSORB_E_NO_DEVICE.  MSORB_INPUT_DIRECT=0 (read when a handle is created) sends
 * every image of that handle down the staged path.
 * ---------------------------------------------------------------------------------------------- */
int msorb_host_alloc(size_t bytes, void** out);        /* hipHostMalloc, portable + mapped; enters the table */
int msorb_host_free(void* p);                          /* leaves the table, then hipHostFree */
/* Pageable memory: hipHostRegister (portable + mapped), owned by the table and unpinned by msorb_host_unregister.  Memory the
 * application pinned itself: verified once, here, with hipPointerGetAttributes, and adopted (never unpinned by the library).
 * A range that overlaps an entry is refused. */
int msorb_host_register(void* p, size_t bytes);
int msorb_host_unregister(void* p);
int msorb_host_admitted(const void* p, size_t bytes);  /* 1: [p, p+bytes) lies wholly inside one table entry; else 0 */

/* ------------------------------------------------------------------------------------------------
 * Extractor — replaces ORB_SLAM3::ORBextractor (include/ORBextractor.h:43-109, src/ORBextractor.cc)
 * ---------------------------------------------------------------------------------------------- */
typedef struct msorb_extractor msorb_extractor;

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * (ORBextractor.cc:409-469).  `device` is the HIP device ordinal the handle lives on.  One handle per
 * extractor object; a handle owns its stream, device pyramid and pinned staging and must not be
 * entered concurrently (the reference never does: Frame.cc:122-125 uses one object per eye). */
int msorb_extractor_create(int nfeatures, float scale_factor, int nlevels, int ini_th_fast, int min_th_fast,
                           int device, msorb_extractor** out);
void msorb_extractor_destroy(msorb_extractor* h);

/* Where the level-0 images of the per-frame entries came from (host-memory admission above).  Since ABI 6002. */
typedef struct msorb_input_stats {   /* since the handle was created */
    uint64_t images_direct;    /* level-0 images uploaded straight from the caller's memory */
    uint64_t images_staged;    /* level-0 images copied by the host into the handle's staging plane (msorb_stage_image counts here, at
                                  stage time) */
    uint64_t bytes_staged;     /* bytes those host copies moved (the copies that refill the host's level 0 behind a direct upload —
                                  msorb_pyramid_level — are not in front of the upload and are not counted) */
    uint64_t upload_launches;  /* kernel launches / hipMemcpyAsync calls that moved level-0 images to the device */
} msorb_input_stats;
int msorb_extractor_input_stats(const msorb_extractor* h, msorb_input_stats* out);

/* GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares
 * (ORBextractor.h:61-81) and mnFeaturesPerLevel; each array has nlevels entries; NULL = skip. */
int msorb_extractor_tables(const msorb_extractor* h, float* scale, float* inv_scale, float* sigma2,
                           float* inv_sigma2, int* features_per_level);

/* Upper bound on keypoints one image can return: nfeatures + 19*nlevels — a level overshoots its quota by at most 3 (SURVEY.md §8a
 * a5), or returns the 4 * nIni children of the quadtree's unconditional first pass when its quota is smaller than that (nIni =
 * round(width / height) <= 4). */
int msorb_extractor_capacity(const msorb_extractor* h);

/* ORBextractor::operator()(image, mask, keypoints, descriptors, vLappingArea) (ORBextractor.cc:1086-1168)
 * on one HOST image (8-bit, 1 channel, `stride` bytes per row).  Writes *n_keypoints keypoints
 * (reference order: keypoints outside [lap0,lap1] from the front, inside from the back) and
 * *n_keypoints x 32 descriptor bytes into caller buffers of `capacity` rows; *mono_index is the
 * operator()'s return value.  Returns MSORB_E_EMPTY for rows==0||cols==0||image==NULL. */
int msorb_extract(msorb_extractor* h, const uint8_t* image, int rows, int cols, size_t stride, int lap0, int lap1,
                  msorb_keypoint* keypoints, uint8_t* descriptors, int capacity, int* n_keypoints,
                  int* mono_index);

/* One stereo frame in one call — what Frame::Frame(imLeft, imRight, ...) does with two extractor threads and
 * ComputeStereoMatches (Frame.cc:119-137): both images go through the batch pipeline together, the stereo association
 * (Frame.cc:743-913, median rejection included) runs on the device-resident outputs, and keypoints, descriptors,
 * mvuRight and mvDepth come back with a single synchronisation.  Lapping areas are 0 (rectified stereo).  Results are
 * identical to two msorb_extract calls followed by msorb_stereo_matches.  capacity = entries available in each of the
 * caller's arrays (>= msorb_extractor_capacity). */
int msorb_extract_stereo(msorb_extractor* h, const uint8_t* left, const uint8_t* right, int rows, int cols,
                         size_t stride_left, size_t stride_right, float mb, float mbf, msorb_keypoint* kps_left,
                         uint8_t* desc_left, int* n_left, msorb_keypoint* kps_right, uint8_t* desc_right, int* n_right,
                         int capacity, float* u_right, float* depth, int* n_oob);

/* The same stereo frame with one extractor object per DEVICE — BASELINE configs[3], "left/right images on 2 MI355X, gather of
 * keypoints/descriptors over xGMI".  Replaces the two extractor threads + join of Frame::Frame (Frame.cc:122-127) followed by
 * ComputeStereoMatches (Frame.cc:743-913) when mpORBextractorLeft and mpORBextractorRight (Tracking.cc:595-596) live on
 * different GPUs: `left` and `right` are two distinct handles (same parameters) created on devices A and B.  Each eye runs
 * its kernel chain on its own device; the right eye's keypoints, descriptors, count and pyramid are copied device to device
 * onto A (peer copy over xGMI when A != B), a HIP event orders the two streams, the stereo association runs on A and one
 * block comes back after one synchronisation.  A == B (two handles on one device) is allowed and takes the same path.
 * Results are identical to msorb_extract_stereo / to two msorb_extract calls + msorb_stereo_matches. */
int msorb_extract_stereo_split(msorb_extractor* left, msorb_extractor* right, const uint8_t* img_left,
                               const uint8_t* img_right, int rows, int cols, size_t stride_left, size_t stride_right,
                               float mb, float mbf, msorb_keypoint* kps_left, uint8_t* desc_left, int* n_left,
                               msorb_keypoint* kps_right, uint8_t* desc_right, int* n_right, int capacity, float* u_right,
                               float* depth, int* n_oob);

/* ComputePyramid (ORBextractor.cc:1170-1195) alone over n_images DEVICE-resident images (arguments as msorb_extract_batch):
 * fills the handle's pyramid, asynchronously on its stream, so that msorb_stereo_matches_split can read it.  Used on the
 * device that runs the stereo association when only the other eye's keypoints / descriptors were gathered (60 B per
 * keypoint) and its levels (1.5 MB per KITTI image) are rebuilt locally instead of being moved. */
int msorb_pyramid_batch(msorb_extractor* h, const uint8_t* d_images, int n_images, int rows, int cols, size_t row_stride,
                        size_t image_stride);

/* mvImagePyramid[level] (ORBextractor.h:83) of the last msorb_extract() call as a host-visible plane
 * (interior pixels; the 19-px border of ORBextractor.cc:1185-1191 is not materialised).  The memory
 * is owned by the handle and valid until the next extract call.  Without msorb_extractor_set_host_pyramid the first
 * call after an extraction copies the whole pyramid synchronously (8 x hipMemcpy2D).  Level 0 is the handle's copy also when the
 * image was read in place from admitted memory (never the caller's pointer): with msorb_extractor_set_host_pyramid the host
 * copies it while the device works, otherwise it comes back from the device with the other levels. */
int msorb_pyramid_level(msorb_extractor* h, int level, const uint8_t** data, int* rows, int* cols, size_t* stride);

/* enable != 0: every msorb_extract() call also brings levels 1.. of the pyramid to pinned host memory, with ONE asynchronous
 * copy on a stream of its own that starts when the pyramid kernels are done and overlaps FAST / quadtree / describe
 * (level 0 is the staged input image); msorb_pyramid_level then only hands out pointers.  For callers that keep reading
 * mvImagePyramid on the host (an unchanged Frame::ComputeStereoMatches, Frame.cc:840-855).  Default off. */
int msorb_extractor_set_host_pyramid(msorb_extractor* h, int enable);

/* TWO images of the same size through ONE kernel chain (the batch pipeline with two images) — what the two extractor threads of
 * Frame::Frame (Frame.cc:122-125) compute with two concurrent operator() calls, for callers that can hand both images over at
 * once WITHOUT the stereo match (msorb_extract_stereo is the call that also matches).  0.159 ms per pair against 2 x 0.13 for
 * two calls.  (A rendezvous of the two eye threads inside the drop-in class onto this call was measured and retired:
 * tools/experiments/README.md.)  Both images share the lapping area [lap0, lap1] (rectified stereo: 0, 0).  Results identical to two
 * msorb_extract calls on two handles.  With msorb_extractor_set_host_pyramid the levels 1.. of BOTH pyramids come back to pinned
 * memory as in msorb_extract (msorb_pyramid_level_image).  capacity = entries available in each of the caller's arrays.
 * staged: bit 0 / bit 1 = image_a / image_b is a pointer msorb_stage_image returned (from ANY handle on this device, with the
 * same geometry): the image already lies in pinned memory at the library's row pitch and is uploaded from there. */
int msorb_extract_pair(msorb_extractor* h, const uint8_t* image_a, const uint8_t* image_b, int rows, int cols, size_t stride_a,
                       size_t stride_b, int lap0, int lap1, msorb_keypoint* kps_a, uint8_t* desc_a, int* n_a, int* mono_a,
                       msorb_keypoint* kps_b, uint8_t* desc_b, int* n_b, int* mono_b, int capacity, int staged);
/* Copies a host image into the handle's pinned staging plane (what msorb_extract does first) and returns that plane: *pinned
 * (valid until the handle's next stage / extract call), *pitch its row pitch.  msorb_extract on the SAME handle recognises
 * the pointer and skips its own copy; msorb_extract_pair takes it with the `staged` bits. */
int msorb_stage_image(msorb_extractor* h, const uint8_t* image, int rows, int cols, size_t stride, const uint8_t** pinned, size_t* pitch);
/* msorb_pyramid_level for image 0 / 1 of the last msorb_extract_pair call (image 0 only after any other extract call). */
int msorb_pyramid_level_image(msorb_extractor* h, int image, int level, const uint8_t** data, int* rows, int* cols, size_t* stride);

/* The OpenCV primitives the extractor restates (resize, GaussianBlur, fastAtan2) are un-vendored dependencies of the reference
 * (CMakeLists.txt:35: OpenCV >= 4.4, no pinned version).  Their semantics follow SURVEY.md Appendix A; the three places where
 * a real OpenCV build could differ — and the one float expression of the reference itself whose rounding its COMPILER decides
 * (brief_tap) — are ONE runtime-selectable table, in the kernels (here) and in the oracle
 * (oracle/cvprims.h Semantics) alike — if a pin run (tools/pin_opencv.py) disagrees with a default, the fix is this call:
 *   gauss_taps       Q8 taps of GaussianBlur(7x7, sigma 2) (ORBextractor.cc:1133).  Default {18,34,48,56,48,34,18}: the
 *                    bit-exact fixed-point path of OpenCV >= 4.2; sum(taps) <= 257.  Other taps run the generic blur kernels.
 *   resize_rounding  vertical pass of resize(INTER_LINEAR, 8U) (ORBextractor.cc:1183).  0 (default): VResizeLinear<uchar>,
 *                    ((b0*(S0>>4))>>16 + (b1*(S1>>4))>>16 + 2) >> 2;  1: the generic FixedPtCast form (S0*b0 + S1*b1 + (1<<21)) >> 22
 *                    (generic resize kernel).
 *   atan2_fma        polynomial of fastAtan2 (ORBextractor.cc:102).  0 (default): separate multiply / add (x86-64 baseline
 *                    build); 1: contracted Horner steps (aarch64, -ffp-contract=fast builds).
 *   brief_tap        the rotated rBRIEF tap cvRound(x*b + y*a), cvRound(x*a - y*b) (ORBextractor.cc:117-119), built with -O3
 *                    -march=native (CMakeLists.txt:10-13), i.e. with whatever contraction that compiler and target choose.
 *                    0 (default): the FIRST product fused, fma(x, b, y*a) / fma(x, a, -(y*b)) — g++ and clang on an FMA target
 *                    (tools/probe_brief_tap.cc, compiled with the reference's flags, prints which one a given build has);
 *                    1: the SECOND product fused, fma(y, a, x*b) / fma(-y, b, x*a);  2: no contraction (a target without FMA,
 *                    -ffp-contract=off).  The conventions differ on about 3 of 10^7 (pattern point, angle) pairs
 *                    (tests/test_semantics_variants.py counts them).
 * sem == NULL restores the defaults.  Applies to every later call on the handle. */
typedef struct msorb_semantics {
    int gauss_taps[7];
    int resize_rounding;
    int atan2_fma;
    int brief_tap;   /* since ABI 6000 */
} msorb_semantics;
int msorb_extractor_set_semantics(msorb_extractor* h, const msorb_semantics* sem);

/* Batched operator() over n_images same-sized DEVICE-resident images (image i at d_images +
 * i*image_stride, rows of row_stride bytes).  Outputs stay on the device: image i's keypoints at
 * d_keypoints + i*capacity, descriptors at d_descriptors + i*capacity*32.  h_counts[i] / h_mono[i]
 * (host arrays, n_images entries, h_mono may be NULL) receive n_keypoints / mono_index.
 * Level 0 is read in place from d_images (it must stay valid until the call returns); rows that are not 4-byte
 * aligned work too — big batches of them (>= 128 images) are first copied into aligned planes owned by the handle,
 * which is faster than running the byte-granular kernel variants (1.88 vs 2.08 ms per 256 KITTI images; 1.72 ms with a
 * 64-byte row pitch). */
int msorb_extract_batch(msorb_extractor* h, const uint8_t* d_images, int n_images, int rows, int cols,
                        size_t row_stride, size_t image_stride, int lap0, int lap1, msorb_keypoint* d_keypoints,
                        uint8_t* d_descriptors, int capacity, int* h_counts, int* h_mono);

/* msorb_extract_batch in two halves: _submit enqueues the whole chain on the handle's streams and returns, _wait blocks until
 * it has finished and hands out the counts (same arrays and error codes as msorb_extract_batch).  One batch per handle may be
 * pending; a caller that alternates two handles keeps the GPU busy across batch boundaries (bench.py does: the next batch's
 * pyramid / FAST run under the previous batch's quadtree / descriptor tail).  The output arrays and the input images must
 * stay untouched until _wait returns.  No reference counterpart: the reference processes one frame at a time. */
int msorb_extract_batch_submit(msorb_extractor* h, const uint8_t* d_images, int n_images, int rows, int cols,
                               size_t row_stride, size_t image_stride, int lap0, int lap1, msorb_keypoint* d_keypoints,
                               uint8_t* d_descriptors, int capacity);
int msorb_extract_batch_wait(msorb_extractor* h, int* h_counts, int* h_mono_index);

/* Stage timing of the last batch call, measured with HIP events on the handle's stream.
 * enable!=0 switches recording on.  Stage order: MSORB_STAGE_* below; ms[] has MSORB_N_STAGES slots. */
#define MSORB_STAGE_PYRAMID 0
#define MSORB_STAGE_FAST 1
#define MSORB_STAGE_COMPACT 2
#define MSORB_STAGE_BLUR 3
#define MSORB_STAGE_SELECT 4   /* device quadtree + output layout (MSORB_QUADTREE=host: D2H candidates + host quadtree + H2D, wall time) */
#define MSORB_STAGE_DESCRIBE 5 /* IC-angle + rBRIEF */
#define MSORB_N_STAGES 6
int msorb_extractor_set_profiling(msorb_extractor* h, int enable);
/* Execution shape of msorb_extract_batch: number of concurrently scheduled sub-batches (1..4, default 2; batches
 * of fewer than 16 images always use 1) and whether the blur runs on a second stream (default yes).  (1, 0) runs
 * every kernel alone on the GPU — the setting used for per-kernel roofline measurements. */
int msorb_extractor_set_overlap(msorb_extractor* h, int sub_batches, int blur_on_second_stream);
int msorb_extractor_stage_ms(const msorb_extractor* h, float* ms);

/* Test/inspection hooks (device -> host copies of intermediate products of the last call). */
int msorb_debug_level_size(const msorb_extractor* h, int level, int* rows, int* cols);
int msorb_debug_copy_level(msorb_extractor* h, int image, int level, int blurred, uint8_t* dst /* rows*cols */);
/* FAST candidates handed to the quadtree (vToDistributeKeys, ORBextractor.cc:795-869) of one image
 * and level, reference order; coordinates relative to (16,16); xyscore[3*i..3*i+2]. */
int msorb_debug_candidates(msorb_extractor* h, int image, int level, int* xyscore, int capacity, int* n);
/* The tables describe_kernel reads, copied back FROM THE DEVICE's constant memory: the 256 x 4 rBRIEF pattern (bit_pattern_31_,
 * ORBextractor.cc:149-406) and umax[16] (:453-468).  For tests that hold what the chip holds to constants recorded independently
 * of this library's sources (tests/golden/reference_constants.json).  Since ABI 6000. */
int msorb_debug_patch_tables(msorb_extractor* h, int8_t* pattern /* 1024 */, int8_t* umax /* 16 */);
/* The std::sort restatement of DistributeOctTree's careful loop (ORBextractor.cc:700: std::sort(vPrevSizeAndPointerToNode, compareNodes),
 * unstable — libstdc++'s introsort decides the order of equal keys, and with it which nodes are split before the quota is reached)
 * ALONE, as the selection kernels run it, on n <= 4000 explicit keys: frame_form != 0 the 1024-thread form of single frames
 * (ranges of <= 64 items sorted in the lanes of one wave; | 2: without that, round 5's form), 0 the 256-thread form of batches.
 * order[i] = input position of the item that ends at position i; sorted_keys and sort_us (the sort alone, timed on the device's
 * constant clock) may be NULL.  Since ABI 6000. */
int msorb_debug_std_sort(int device, const uint32_t* keys, int n, int frame_form, uint32_t* order, uint32_t* sorted_keys, float* sort_us);
/* Host-only: the per-thread table of the FAST kernel (one 16-byte record per thread of every class of cells with equal records) as
 * an extractor of these parameters builds it for a rows x cols image and workgroups of `threads` (128 or 256) threads.  cells receives
 * MSORB_FAST_CELL_FIELDS int32 per cell, in cell order: level, x0, y0, rw, rh, G, ndw, g_magic, R128, R256, by_wave[0], by_wave[1], spw,
 * rw128, yw128, rw256, yw256, first record of the cell's class, level width, level height.  records receives 4 uint32 per record:
 * staging store offset, quick-test window offset, column mask, rows | work-list base << 16.  The counts are written even when a
 * capacity is too small (MSORB_E_CAPACITY).  Needs no GPU. */
#define MSORB_FAST_CELL_FIELDS 20
int msorb_debug_fast_thread_table(int rows, int cols, int nfeatures, float scale_factor, int nlevels, int threads,
                                  int32_t* cells, int cell_capacity, int* n_cells,
                                  uint32_t* records, int record_capacity, int* n_records, int* n_classes);
/* The cosine and sine describe_kernel steers the rBRIEF pattern with (ORBextractor.cc:112: a = cos(angle * factorPI), b = sin(..)),
 * ALONE, on n <= 2^26 explicit angles in degrees: the same device function the kernel calls, so every bit of the device build of the
 * glibc sinf / cosf restatement can be held to the installed libm (inside the extractor a and b are seen only through the rounded
 * tap positions).  Appended to ABI 6002: MSORB_ABI_VERSION is unchanged, a caller that needs the entry asks the loader for it. */
int msorb_debug_cos_sin(int device, const float* angles_deg, int n, float* cos_out, float* sin_out);
/* One shared Lie-group primitive of the optimisers (the rotation arithmetic of se3_device.h, sim3_opt_device.h, essential_graph_device.h,
 * essential_graph4_device.h, inertial_device.h and mlpnp_device.h), ALONE, on n <= 2^20 explicit records: the functions the
 * optimisation kernels call, compiled with the library's flags against the device's libm.  op (0..21) and the record layouts are
 * listed in ms-slam_amd/csrc/lie_probe_device.h: 16 doubles in (80 for op 16, bias_corrected) and 24 doubles out per record, float
 * functions taking exactly representable floats and returning floats widened.  MSORB_E_INVALID, with out untouched, for a null
 * pointer with n > 0, a negative n or an unknown op; n == 0 launches nothing.  Two calls on the same input return the same bits.
 * Appended to ABI 6002: MSORB_ABI_VERSION is unchanged, a caller that needs the entry asks the loader for it. */
int msorb_debug_lie(int device, int op, const double* in, int n, double* out);
/* One small dense decomposition of the RANSAC solvers and optimisers (the 3x3 SVD, inverse and determinant and the 9-column null
 * vector of two_view_device.h, the 4x4 null vector of new_points_device.h, the 4x4 eigenvector and quaternion rotation of
 * sim3_device.h, the rank, eigenvectors, 6x6 solve and 12 / 9-column null vector of mlpnp_device.h, ldlt_factor / ldlt_apply of
 * inertial_device.h), ALONE, on n <= 2^20 explicit records: the functions the kernels call, compiled with the library's flags.  The
 * one-thread routines run a thread per record; the two cooperative null vectors run a workgroup per record, of the size and on the
 * shared work of the kernel that calls them, and report how many lanes returned other bits than lane 0.  op (0..13), the record
 * widths and layouts are listed in ms-slam_amd/csrc/decomp_probe_device.h; 24 doubles out per record, float functions taking exactly
 * representable floats and returning floats widened.  MSORB_E_INVALID, with out untouched, for a null pointer with n > 0, a negative
 * n or an unknown op; n == 0 launches nothing.  Two calls on the same input return the same bits.
 * Appended to ABI 6002: MSORB_ABI_VERSION is unchanged, a caller that needs the entry asks the loader for it. */
int msorb_debug_decomp(int device, int op, const double* in, int n, double* out);
/* Host-only: DistributeOctTree (ORBextractor.cc:555-779) on explicit candidates; writes the indices of
 * the kept candidates in result order.  Needs no GPU. */
int msorb_distribute_quadtree(const uint16_t* xs, const uint16_t* ys, const uint16_t* scores, int n, int min_x,
                              int max_x, int min_y, int max_y, int n_features, int* kept_idx, int capacity,
                              int* n_kept);

/* ------------------------------------------------------------------------------------------------
 * Matcher — the data-parallel core of ORB_SLAM3::ORBmatcher (include/ORBmatcher.h:36-112,
 * src/ORBmatcher.cc) and Frame::ComputeStereoMatches (src/Frame.cc:743-913) on flat arrays.
 * The graph/mutex side of the reference (shared_ptr<MapPoint>, Observations(), pose projection with
 * Sophus/Eigen) stays in the caller; these entries start from projected coordinates and descriptor
 * arrays and return exactly the assignments the reference's loops would make (same candidate sets,
 * same scan order, same tie-breaks, same sequential side effects).
 * ---------------------------------------------------------------------------------------------- */
typedef struct msorb_frame msorb_frame;

/* A frame's features on the device plus its 64x48 feature grid.  One handle per thread of use. */
int msorb_frame_create(int device, msorb_frame** out);
void msorb_frame_destroy(msorb_frame* f);

/* Frame members the matcher reads: mvKeysUn, mDescriptors, mvuRight (NULL = all -1), image bounds
 * mnMinX..mnMaxY, mvScaleFactors.  Builds mGrid like Frame::AssignFeaturesToGrid (Frame.cc:385-416,
 * PosInGrid :657-667) — on the device, from the uploaded features (frame_grid_kernel).  Host arrays.  At most 32768 keypoints
 * per frame on gfx950 (what one workgroup's 160 KB of LDS sorts; MSORB_E_CAPACITY beyond, decided before the handle is
 * touched).  A call that fails later (allocation, HIP error) leaves the handle EMPTY: no keypoints, an empty grid. */
int msorb_frame_set(msorb_frame* f, const msorb_keypoint* keypoints, int n, const uint8_t* descriptors,
                    const float* u_right, float min_x, float max_x, float min_y, float max_y,
                    const float* scale_factors, int nlevels);

/* Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) (Frame.cc:589-655): indices in the reference's
 * order (cells ix outer / iy inner, insertion order inside a cell).  Host-side walk of the same grid
 * the kernels use. */
int msorb_frame_features_in_area(const msorb_frame* f, float x, float y, float r, int min_level, int max_level,
                                 int* out_idx, int capacity, int* n);

/* Telemetry of the searches that replay sequential claims on the host (all SearchByProjection forms on a frame / KeyFrame
 * handle): returns the number of device rounds the LAST such search on `f` needed — 1 unless a query's candidate list (8
 * entries) was exhausted by earlier claims, in which case the kernel is re-run from that query on (at most one round per
 * query) —, and through the optional pointers the totals since msorb_frame_create. */
int msorb_frame_search_rounds(const msorb_frame* f, long long* total_rounds, long long* total_searches);

/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint>&, th, bFarPoints, thFarPoints)
 * (ORBmatcher.cc:43-142, rectified branch).  Map-point table of m entries visited in index order:
 *   track_in_view=mbTrackInView  bad=isBad()  sparsified=mbSparsified  proj_x/proj_y/proj_xr=mTrackProjX/Y/XR
 *   track_depth=mTrackDepth  level=mnTrackScaleLevel  view_cos=mTrackViewCos  mp_desc=GetDescriptor() (m x 32)
 *   obs=Observations().
 * frame_mp[n]: F.mvpMapPoints as table indices (-1 = none, every entry < m), updated in place.  *nmatches = return value. */
int msorb_search_by_projection_mps(msorb_frame* f, int m, const uint8_t* track_in_view, const uint8_t* bad,
                                   const uint8_t* sparsified, const float* proj_x, const float* proj_y,
                                   const float* proj_xr, const float* track_depth, const int* level,
                                   const float* view_cos, const uint8_t* mp_desc, const int* obs, int* frame_mp,
                                   float th, int far_points, float th_far_points, float nnratio, int* nmatches);

/* The same search on a TWO-CAMERA frame (F.Nleft != -1, the KannalaBrandt8 stereo rig): ORBmatcher.cc:43-213 with both arms —
 * per map point a left pass (:61-142; no mvuRight test for such a frame, :92) and a right pass (:144-210; radius not scaled by th,
 * no mbSparsified bypass), coupled through mvLeftToRightMatch / mvRightToLeftMatch (a match on one side also claims the stereo
 * partner on the other, :130-134 / :196-200) and through the `continue` of a failed left ratio test (:125-126: no right pass for
 * that point).  `left` / `right`: two msorb_frame handles on one device, set from F.mvKeys[0, Nleft) / F.mvKeysRight with their
 * descriptor rows and WITHOUT mvuRight (what Frame::GetFeaturesInArea(..., bRight) walks, Frame.cc:589-655).  The table has, beside
 * the entries of msorb_search_by_projection_mps, the right camera's scratch: track_in_view_r=mbTrackInViewR,
 * proj_xr / proj_yr=mTrackProjXR / mTrackProjYR, level_r=mnTrackScaleLevelR (-1: no right pass), view_cos_r=mTrackViewCosR.
 * left_to_right[n_left] / right_to_left[n_right] = F.mvLeftToRightMatch / F.mvRightToLeftMatch (-1 none).
 * frame_mp[n_left + n_right] = F.mvpMapPoints as table indices, updated in place.  Since ABI 6000. */
int msorb_search_by_projection_mps_rig(msorb_frame* left, msorb_frame* right, int m, const uint8_t* track_in_view,
                                       const uint8_t* track_in_view_r, const uint8_t* bad, const uint8_t* sparsified, const float* proj_x,
                                       const float* proj_y, const float* proj_xr, const float* proj_yr, const float* track_depth,
                                       const int* level, const int* level_r, const float* view_cos, const float* view_cos_r,
                                       const uint8_t* mp_desc, const int* obs, const int* left_to_right, const int* right_to_left,
                                       int* frame_mp, float th, int far_points, float th_far_points, float nnratio, int* nmatches);

/* The window search on its own, for the SearchByProjection variants that keep their accept rules in the caller
 * (KeyFrame / Sim3 / relocalisation forms, ORBmatcher.cc:423-753, 2154-2275): for each query the 4 nearest
 * descriptors among GetFeaturesInArea(x, y, r, min_level, max_level) in the reference's scan order (ties ->
 * earlier in the scan), skipping keypoints flagged in occupied[n] when skip_occupied[i] != 0 and keypoints whose
 * mvuRight differs from ur[i] by more than r[i] (ur == NULL disables nothing: pass a frame without mvuRight).
 * best_idx / best_dist have 4 entries per query (-1 / 256 = none). */
int msorb_window_top4(msorb_frame* f, int n_queries, const float* x, const float* y, const float* r, const float* ur,
                      const int* min_level, const int* max_level, const uint8_t* skip_occupied, const uint8_t* query_desc,
                      const uint8_t* occupied, int* best_idx, int* best_dist);

/* The search of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = false) (ORBmatcher.cc:1404-1597; LocalMapping::
 * SearchInNeighbors, LocalMapping.cc:793-826): for every map point the best keypoint of the KeyFrame inside
 * GetFeaturesInArea(u, v, radius) (KeyFrame.cc:796-845) at level predicted-1 .. predicted (:1513-1514) that passes the
 * reprojection-error gate (:1517-1545: e2 * mvInvLevelSigma2[level] <= 7.8 with the stereo term when mvuRight >= 0,
 * <= 5.99 otherwise), first strict minimum in scan order (:1555-1559).  `f` = the KeyFrame loaded with msorb_frame_set: mvKeysUn,
 * mDescriptors, mvuRight, image bounds, scale factors.  Per point: valid (it survived :1436-1497), u, v (projection),
 * ur (u - bf*invz), predicted_level (PredictScale), radius (th * mvScaleFactors[level]), mp_desc.  best_idx / best_dist
 * (-1 / 256 = none).  What happens with a match (Replace / AddObservation, :1563-1588) mutates the map and stays with
 * the caller, which also re-checks isBad() / IsInKeyFrame() at that time like the reference's loop does. */
int msorb_fuse_search(msorb_frame* f, const float* inv_level_sigma2, int n_levels, int n, const uint8_t* valid,
                      const float* u, const float* v, const float* ur, const int* predicted_level, const float* radius,
                      const uint8_t* mp_desc, int* best_idx, int* best_dist);

/* The same search for ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = true) on a two-camera KeyFrame (NLeft != -1;
 * LocalMapping.cc:794-795, 825-826).  There the window is KeyFrame::GetFeaturesInArea(u, v, radius, true): the RIGHT camera's
 * grid and keypoints (KeyFrame.cc:826-836) — `f` = that camera loaded with msorb_frame_set — while the level band and the
 * reprojection-error gate read pKF->GetKeyPoint(idx) and pKF->GetuRight(idx) with the right-camera index idx as it comes out
 * of the grid (ORBmatcher.cc:1509-1545; `idx += NLeft` follows at :1547), i.e. mvKeys[idx] for idx < NLeft and
 * mvKeysRight[idx - NLeft] beyond (KeyFrame.h:377-385).  gate_kps[f->N] / gate_uright[f->N] are those values per right-camera
 * index (gate_uright NULL = -1 everywhere); everything else as msorb_fuse_search, best_idx in right-camera indices (the caller adds
 * NLeft).  With gate_kps = the frame's own keypoints and gate_uright = its mvuRight this is msorb_fuse_search.  Since ABI 6001. */
int msorb_fuse_search_gated(msorb_frame* f, const msorb_keypoint* gate_kps, const float* gate_uright, const float* inv_level_sigma2,
                            int n_levels, int n, const uint8_t* valid, const float* u, const float* v, const float* ur,
                            const int* predicted_level, const float* radius, const uint8_t* mp_desc, int* best_idx, int* best_dist);

/* ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th, bMono) (ORBmatcher.cc:1941-2057,
 * 2129-2152) from the projected coordinates on.  Per last-frame keypoint i: valid (map point present, not
 * outlier, positive depth, inside the image), u,v (projection), ur (u - mbf/z), last_octave, last_angle,
 * mp_desc (n_last x 32), last_mp (id stored into cur_mp), obs[id] = Observations() of map point id, n_obs entries: every
 * id in last_mp (of a valid entry) and in cur_mp must be < n_obs (MSORB_E_INVALID otherwise).  cur_mp[n] in/out. */
int msorb_search_by_projection_frames(msorb_frame* cur, int n_last, const uint8_t* valid, const float* u,
                                      const float* v, const float* ur, const int* last_octave,
                                      const float* last_angle, const uint8_t* mp_desc, const int* last_mp,
                                      const int* obs, int n_obs, int* cur_mp, float th, int forward, int backward,
                                      int check_orientation, int* nmatches);

/* The same search on a two-camera CurrentFrame (Nleft != -1; ORBmatcher.cc:1941-2152 with the right-camera arm :2059-2124), from
 * the projected coordinates on.  left / right: the current frame's two cameras as in msorb_search_by_projection_mps_rig.  Per
 * last-frame keypoint: valid (the tests of :1962-1983, on the LEFT projection), u, v (left camera), u_r, v_r
 * (mpCamera->project(GetRelativePoseTrl() * x3Dc), :2060-2061), last_octave / last_angle (the Nleft-aware keypoint of LastFrame).
 * cur_mp[n_left + n_right] in / out.  The right window of a keypoint is searched only when its left window held a candidate
 * (:2003-2004); one rotation histogram over both arms.  Since ABI 6000. */
int msorb_search_by_projection_frames_rig(msorb_frame* left, msorb_frame* right, int n_last, const uint8_t* valid, const float* u,
                                          const float* v, const float* u_r, const float* v_r, const int* last_octave,
                                          const float* last_angle, const uint8_t* mp_desc, const int* last_mp, const int* obs, int n_obs,
                                          int* cur_mp, float th, int forward, int backward, int check_orientation, int* nmatches);

/* ORBmatcher::SearchByProjection(Frame& Current, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:2154-2275,
 * Tracking::Relocalization :3672, :3695) from the projected coordinates on.  Per map point of the KeyFrame that the
 * loop reaches (not bad, not in sAlreadyFound, inside the image, distance inside the scale pyramid, :2173-2196):
 * valid, u, v, predicted_level (PredictScale, :2198), kf_angle (pKF->GetKeyUn(i).angle, :2237), mp_desc, mp_id (stored
 * into cur_mp).  A keypoint of the frame that holds ANY map point is never taken (:2214-2215); accept bestDist <=
 * orb_dist (:2229); cur_mp[n] in/out (-1 = none). */
int msorb_search_by_projection_kf(msorb_frame* cur, int n, const uint8_t* valid, const float* u, const float* v,
                                  const int* predicted_level, const float* kf_angle, const uint8_t* mp_desc,
                                  const int* mp_id, int* cur_mp, float th, int orb_dist, int check_orientation,
                                  int* nmatches);

/* The Sim3 / loop-closing window searches that claim keypoints: SearchByProjection(pKF, Scw, vpPoints, vpMatched, th,
 * ratioHamming) (ORBmatcher.cc:423-530) and the (pKF, Scw, vpPoints, vpPointsKFs, ...) form (:639-753), from the projected
 * coordinates on (SearchByProjectionLoop, :532-637, has different rules: msorb_search_by_projection_loop).  `kf` = the KeyFrame loaded with msorb_frame_set.  Per candidate point
 * that passed :446-480: valid, u, v, predicted_level, mp_desc, mp_id.  Keypoints with matched[idx] >= 0 are skipped
 * (:499-500), level band predicted-1 .. predicted (:505-507), first strict minimum, accepted when
 * (float)bestDist <= max_dist (= TH_LOW * ratioHamming, :521) and then claimed: matched[bestIdx] = mp_id (in/out).
 * The claim-free searches of Fuse(pKF, Scw, ...) (:1599-1716) and SearchBySim3 (:1718-1939) have entries of their own:
 * msorb_fuse_sim3_search and msorb_search_by_sim3. */
int msorb_search_by_projection_sim3(msorb_frame* kf, int n, const uint8_t* valid, const float* u, const float* v,
                                    const int* predicted_level, const uint8_t* mp_desc, const int* mp_id, int* matched,
                                    float th, float max_dist, int* nmatches);

/* ORBmatcher::SearchByProjectionLoop(pKF, Scw, vpPoints, vpMatched, vpMatchedKF, th, ratioHamming) (ORBmatcher.cc:532-637;
 * LoopClosing::DetectCommonRegionsFromBoW :744,:753) from the projected coordinates on.  Per candidate point that passed
 * :555-588 (not bad, vpMatched[iMP] still empty, positive depth, inside the image, distance, viewing angle): valid, u, v,
 * predicted_level, mp_desc.  A keypoint is a candidate only when it holds a good map point (train_ok[idx] =
 * vpMapPointsToMatch[idx] && !isBad(), :609-610), level band predicted-1 .. predicted+1 (:613), first strict minimum,
 * accepted when bestDist <= max_dist (= TH_LOW * ratioHamming, :626).  Results are per POINT and independent of each other:
 * best_idx[i] = the keypoint whose map point becomes vpMatched[iMP], or -1; *nmatches = the return value. */
int msorb_search_by_projection_loop(msorb_frame* kf, int n, const uint8_t* valid, const float* u, const float* v,
                                    const int* predicted_level, const uint8_t* mp_desc, const uint8_t* train_ok, float th,
                                    float max_dist, int* best_idx, int* nmatches);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (ORBmatcher.cc:1718-1939; LoopClosing) from the projected
 * coordinates on.  kf1 / kf2 = the two KeyFrames loaded with msorb_frame_set (n1 / n2 = their feature counts).  Per map
 * point i1 of pKF1 that pass 1 reaches (:1760-1794: present, not already matched, not bad, positive depth after S21 * T1w,
 * inside pKF2's image, distance inside the scale pyramid): valid1, u1, v1 (projection into pKF2), level1 =
 * PredictScale(dist3D, pKF2), desc1 = GetDescriptor(); symmetric arrays for pass 2 (:1850-1885).  Each pass searches
 * GetFeaturesInArea(u, v, th * mvScaleFactors[level]) of the other KeyFrame at levels level-1 .. level, first strict
 * minimum, accepted when bestDist <= TH_HIGH (:1843-1846, :1915-1918); match12[i1] = idx2 when both passes agree
 * (:1922-1937), else -1; *nfound = the return value.  vpMatches12[i1] = vpMapPoints2[match12[i1]] stays with the caller. */
int msorb_search_by_sim3(msorb_frame* kf1, msorb_frame* kf2, int n1, const uint8_t* valid1, const float* u1, const float* v1,
                         const int* level1, const uint8_t* desc1, int n2, const uint8_t* valid2, const float* u2,
                         const float* v2, const int* level2, const uint8_t* desc2, float th, int* match12, int* nfound);

/* The search of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1599-1716; LoopClosing::
 * SearchAndFuse): for every candidate point that passed :1622-1656 (valid, u, v, predicted_level, mp_desc) the best keypoint
 * of the KeyFrame inside GetFeaturesInArea(u, v, th * mvScaleFactors[level]) at levels level-1 .. level, first strict
 * minimum, NO reprojection-error gate (unlike msorb_fuse_search).  best_idx -1 / best_dist INT_MAX = none.  The accept rule
 * bestDist <= TH_LOW and what follows (vpReplacePoint / AddObservation / AddMapPoint, :1698-1713) stay with the caller:
 * they read and mutate the map sequentially. */
int msorb_fuse_sim3_search(msorb_frame* kf, int n, const uint8_t* valid, const float* u, const float* v,
                           const int* predicted_level, const uint8_t* mp_desc, float th, int* best_idx, int* best_dist);

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cc:755-870; monocular
 * initialisation).  f1 / f2 = the two frames loaded with msorb_frame_set (both on one device).  prev_xy = vbPrevMatched
 * (x, y per F1 keypoint; updated in place like :864-867), matches12[N1] = vnMatches12, *nmatches = the return value.  The
 * device evaluates every (level-0 keypoint of F1, candidate of F2 in the window) Hamming distance in the reference's scan
 * order; the sequential rule "a train matched at a smaller or equal distance is skipped" (:791-792), the ratio test, the
 * re-assignment of trains and the rotation histogram are replayed on the host over those lists. */
int msorb_search_for_initialization(msorb_frame* f1, msorb_frame* f2, float* prev_xy, int window_size, float nnratio,
                                    int check_orientation, int* matches12, int* nmatches);

/* Best / second-best Hamming match of each query over an explicit candidate list (CSR: candidates of
 * query i are cand_idx[cand_begin[i] .. cand_begin[i+1])), scanned in list order with strict '<' — the
 * inner loop of SearchByBoW / SearchForTriangulation / Fuse (e.g. ORBmatcher.cc:288-330).  Host arrays. */
int msorb_hamming_top2(int device, const uint8_t* query_desc, int n_queries, const uint8_t* train_desc, int n_train,
                       const int* cand_begin, const int* cand_idx, int* best_idx, int* best_dist, int* second_idx,
                       int* second_dist);

/* Dense brute-force top-2 Hamming match, batched and device resident (the "brute-force Hamming match" of BASELINE.json's
 * metric): for each of n_frames frames, every query row against every train row of the same frame with
 * ORBmatcher::DescriptorDistance (ORBmatcher.cc:2323-2339); candidates scanned in index order with strict '<' (ties -> lowest
 * index).  d_* are DEVICE pointers: descriptors [n_frames][stride][32], counts [n_frames], outputs [n_frames][query_stride]
 * (rows past a frame's query count are not written).  Two formulations with identical results:
 *   MSORB_DENSE_POPCOUNT      v_xor + v_bcnt per dword: BASELINE north_star's formulation ("per-wavefront popcount ... no MFMA"),
 *                             the DEFAULT of every entry that does not take the argument (since ABI 6000)
 *   MSORB_DENSE_MATRIX_CORES  an opt-in variant: distances as int8 dot products (v_mfma_i32_32x32x32_i8; the accumulator is the
 *                             (distance, index) key) — 2.9x the rate of the popcount form, outside the north_star's design rule
 * The launch is repeated `repeats` times on a private stream between two HIP events; *elapsed_ms (may be NULL)
 * receives the total.  max_train <= 2048. */
#define MSORB_DENSE_MATRIX_CORES 0
#define MSORB_DENSE_POPCOUNT 1
int msorb_hamming_dense_top2_batch_ex(int device, const uint8_t* d_query, const uint8_t* d_train, const int* d_n_query,
                                      const int* d_n_train, int n_frames, int query_stride, int train_stride, int max_query,
                                      int max_train, int* d_best_idx, int* d_best_dist, int* d_second_dist, int repeats,
                                      float* elapsed_ms, int formulation);
/* The entry without the formulation argument: MSORB_DENSE_POPCOUNT since ABI 6000 (rounds 1-5 ran the matrix-core variant
 * here; results are identical, only the rate differs). */
int msorb_hamming_dense_top2_batch(int device, const uint8_t* d_query, const uint8_t* d_train, const int* d_n_query,
                                   const int* d_n_train, int n_frames, int query_stride, int train_stride, int max_query,
                                   int max_train, int* d_best_idx, int* d_best_dist, int* d_second_dist, int repeats,
                                   float* elapsed_ms);

/* cv::BFMatcher(cv::NORM_HAMMING).knnMatch(query, train, matches, 2) — the brute-force step of
 * Frame::ComputeStereoFishEyeMatches (Frame.cc:1057-1076: left vs right descriptors of the lapping area) — on HOST arrays of
 * 32-byte rows: best_idx / best_dist = matches[i][0] (trainIdx, distance), second_dist (and second_idx, may be NULL) =
 * matches[i][1]; ties go to the lower train index.  -1 / 256 where the train set has fewer than one / two rows.  The Lowe
 * ratio test and KannalaBrandt8::TriangulateMatches of :1082-1098 stay with the caller (host mirror:
 * msorb_host::ComputeStereoFishEyeMatches).  Runs the popcount formulation of the dense kernel. */
int msorb_knn_match2(int device, const uint8_t* query, int n_query, const uint8_t* train, int n_train, int* best_idx,
                     int* best_dist, int* second_idx, int* second_dist);

/* Frame::ComputeStereoMatches (Frame.cc:743-913).  left/right are the two extractor handles whose last
 * msorb_extract() call produced the images' pyramids (mpORBextractorLeft/Right->mvImagePyramid stay on
 * the device).  Keypoint/descriptor arrays are host arrays as returned by msorb_extract.  Writes
 * mvuRight / mvDepth (n_left entries, -1 = none).  *n_oob counts keypoints whose SAD window would leave
 * the pyramid plane (the reference would hit a CV_Assert there; they are skipped).  The two handles may live on
 * different devices (one extractor object per GPU): the right pyramid is then copied to the left handle's device peer to
 * peer before the kernel runs there. */
int msorb_stereo_matches(msorb_extractor* left, msorb_extractor* right, const msorb_keypoint* kps_left, int n_left,
                         const uint8_t* desc_left, const msorb_keypoint* kps_right, int n_right,
                         const uint8_t* desc_right, float mb, float mbf, float* u_right, float* depth, int* n_oob);

/* ORBmatcher::SearchByBoW — the three forms: (pKF, F, vpMapPointMatches) ORBmatcher.cc:223-421 (pinhole branch,
 * F.Nleft == -1; TrackReferenceKeyFrame Tracking.cc:2727, Relocalization :3585) and the two KeyFrame-KeyFrame forms
 * :872-1016, :1018-1166 (LoopClosing).  One msorb_bow_pair per call of the reference; a batch of pairs (all
 * relocalisation / loop candidates of one frame) is matched by ONE launch, one wavefront per (pair, common node).
 * Set 1 = the queries (pKF / pKF1), set 2 = the trains (F / pKF2):
 *   desc1/desc2     n x 32 descriptor rows
 *   valid1[n1]      1 = the query is visited (map point present and not bad, descriptor not empty, :253-263 /
 *                   :910-920 / :1066-1078)
 *   avail2[n2]      1 = the train may be chosen (:934-944 / :1090-1103); NULL = all (the Frame form, :227)
 *   fvK_*           DBoW2::FeatureVector as CSR: node ids ascending (std::map order), features of node r are
 *                   fvK_feat[fvK_begin[r] .. fvK_begin[r+1]); a feature index appears at most once per vector
 *   angle1/angle2   keypoint angles for the rotation histogram (may be NULL when check_orientation == 0)
 * Outputs: match12[n1] = index of the matched train or -1, match21[n2] (may be NULL) the inverse, nmatches — all
 * after the histogram filter (:396-418).  th_low / inclusive: bestDist1 <= TH_LOW (:332) or bestDist1 < TH_LOW
 * (:959, :1118).  Host arrays; *elapsed_ms (may be NULL) = device time of the launch. */
typedef struct msorb_bow_pair {
    int n1, n2;
    const uint8_t *desc1, *desc2;
    const uint8_t *valid1, *avail2;
    int fv1_nodes;
    const int *fv1_node, *fv1_begin, *fv1_feat;
    int fv2_nodes;
    const int *fv2_node, *fv2_begin, *fv2_feat;
    const float *angle1, *angle2;
    int *match12, *match21;
    int nmatches;
} msorb_bow_pair;
int msorb_search_by_bow(int device, msorb_bow_pair* pairs, int n_pairs, int th_low, int inclusive, float nnratio,
                        int check_orientation, float* elapsed_ms);
/* ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) on a two-camera frame (F.Nleft != -1; ORBmatcher.cc:223-421 with the arms of
 * :276-309 / :357-382): inside a BoW node every KeyFrame feature keeps a best / second over the frame's LEFT features (rows
 * < n_left) and a best over its RIGHT features, each among the features no earlier KeyFrame feature has claimed; the left match as on
 * a one-camera frame (<= th_low, ratio test), the right match at <= th_low WITHOUT a ratio test and only when the left best distance
 * was <= th_low (:330 encloses :357).  pair: set 1 = the KeyFrame (valid1 = map point present and good), set 2 = the frame's
 * n2 = N features, left camera first, angle2 = [mvKeys angles | mvKeysRight angles]; avail2 is not read.  match21[n2] (required):
 * the KeyFrame feature whose map point frame feature j receives, -1 none; match12 (optional): the LEFT partner of each KeyFrame
 * feature; nmatches counts both cameras.  One rotation histogram over both (:338-353, :361-378, :396-418).  Since ABI 6000. */
int msorb_search_by_bow_rig(int device, msorb_bow_pair* pair, int n_left, int th_low, float nnratio, int check_orientation);

/* ORBmatcher::SearchForTriangulation (ORBmatcher.cc:1168-1402) with the geometric test of :1332 —
 * pCamera1->epipolarConstrain(pCamera2, kp1, kp2, R12, t12, sigma1, sigma2) — left to the CALLER: the form for the two-camera
 * KeyFrames of a fisheye rig (:1294-1330 pick one of four relative poses and two camera models per candidate pair;
 * KannalaBrandt8::epipolarConstrain triangulates, KannalaBrandt8.cpp:216-220) and for any camera model this library does not
 * restate.  pair: as msorb_search_by_bow — set 1 = pKF1's N features (valid1 = no map point, stereo when bOnlyStereo, :1237-1247),
 * set 2 = pKF2's (avail2 = the same for pKF2, :1259-1271; NULL = all), the two FeatureVectors, angle1 / angle2 = GetKeyPoint(idx).angle.
 * Per common node and visited query, in the reference's order, the library finds the trains within th_low (TH_LOW) on the device
 * and calls accept(ctx, idx1, idx2) on them — smallest distance first, among equal distances the LATER train first (the scan's
 * `dist > bestDist` rule, :1277, lets a later equal candidate replace an earlier one) — skipping trains an earlier query took,
 * until one passes: that train is the query's match.  accept must be a pure predicate of (idx1, idx2) (the reference's is); it is
 * called on the calling thread, between the device passes and the return.  Not applied: the epipole-distance test of :1283-1291
 * (`!pKF1->mpCamera2` guards it: a caller that wants it puts it into accept).  match12 / match21 / nmatches after the rotation
 * histogram (:1360-1381).  Since ABI 6001. */
typedef int (*msorb_pair_accept)(void* ctx, int idx1, int idx2);
int msorb_search_for_triangulation_cb(int device, msorb_bow_pair* pair, int th_low, int check_orientation, msorb_pair_accept accept,
                                      void* ctx);

/* ORBmatcher::SearchForTriangulation (ORBmatcher.cc:1168-1402; LocalMapping::CreateNewMapPoints, LocalMapping.cc:492)
 * for pinhole KeyFrames without a second camera.  One msorb_triangulation_pair per (mpCurrentKeyFrame, neighbour)
 * call; all neighbours of one CreateNewMapPoints pass are matched by ONE launch.
 *   valid1[n1]   1 = the query is visited: no map point (:1237-1241), stereo when bOnlyStereo (:1245-1247), descriptor
 *                not empty;   avail2[n2]  1 = the train is eligible: no map point, stereo when bOnlyStereo (:1264-1271)
 *   stereo1/2    GetuRight(idx) >= 0 (:1243, :1267)
 *   kp1 / kp2    GetKeyPoint(idx) for every feature (cv::KeyPoint layout: pt, angle and octave are read)
 *   scale_factors2 / level_sigma2_2 [n_levels2]   pKF2->mvScaleFactors / mvLevelSigma2 (:1287, :1332)
 *   F12          K1^-T [t12]x R12 K2^-1, row major, exactly the Eigen expression of Pinhole::epipolarConstrain
 *                (Pinhole.cpp:109-112) — constant per pair, so the caller evaluates it once instead of per candidate
 *   ep           pKF2->mpCamera->project(T2w * pKF1->GetCameraCenter()) (:1177-1181)
 * coarse = bCoarse (:1332 skips the epipolar test).  match12[n1] = vMatches12 after the orientation filter
 * (:1360-1381); nmatches = the return value; vMatchedPairs = the (i, match12[i]) with match12[i] >= 0 in index order. */
typedef struct msorb_triangulation_pair {
    int n1, n2;
    const uint8_t *desc1, *desc2;
    const uint8_t *valid1, *avail2, *stereo1, *stereo2;
    int fv1_nodes;
    const int *fv1_node, *fv1_begin, *fv1_feat;
    int fv2_nodes;
    const int *fv2_node, *fv2_begin, *fv2_feat;
    const msorb_keypoint *kp1, *kp2;
    const float *scale_factors2, *level_sigma2_2;
    int n_levels2;
    float F12[9];
    float ep[2];
    int* match12;
    int nmatches;
} msorb_triangulation_pair;
int msorb_search_for_triangulation(int device, msorb_triangulation_pair* pairs, int n_pairs, int coarse,
                                   int check_orientation, float* elapsed_ms);

/* Resident KeyFrames for the BoW-node searches.  A KeyFrame's descriptors, keypoints and FeatureVector are fixed from
 * KeyFrame::ComputeBoW on (until map sparsification compacts them: remove + add), while it is matched many times — by
 * LocalMapping::CreateNewMapPoints against every neighbour (LocalMapping.cc:430-492), as a relocalisation / loop candidate
 * (Tracking.cc:3577-3600, LoopClosing.cc).  msorb_search_by_bow / msorb_search_for_triangulation stage both sides of every
 * pair on every call; a store keeps them on the device, and a search moves only one flag byte per feature, the (pair,
 * common node) work items and, for the KeyFrame-vs-Frame form, the frame.  Same kernels, same results.  Thread-safe:
 * searches may run concurrently with each other; add / remove wait for running searches. */
typedef struct msorb_kf_store msorb_kf_store;
int msorb_kf_store_create(int device, msorb_kf_store** out);
void msorb_kf_store_destroy(msorb_kf_store* s);
int msorb_kf_store_count(const msorb_kf_store* s);
/* kps = GetAllKeyUn() (pt, angle, octave are used), desc = GetDescriptor(i) rows, fv_* = GetFeatureVector() as CSR (node ids
 * ascending), scale_factors / level_sigma2 = mvScaleFactors / mvLevelSigma2.  *kf_id identifies the KeyFrame in later calls. */
int msorb_kf_store_add(msorb_kf_store* s, int n, const msorb_keypoint* kps, const uint8_t* desc, int fv_nodes, const int* fv_node,
                       const int* fv_begin, const int* fv_feat, const float* scale_factors, const float* level_sigma2, int n_levels,
                       int* kf_id);
/* The KeyFrame's rows and its id go back to the store: the next add takes them (first fit over the freed ranges), so that the
 * store's footprint follows the LIVE KeyFrames of a sequence, not its length (tests/soak_main.cc).  kf_id is invalid afterwards. */
int msorb_kf_store_remove(msorb_kf_store* s, int kf_id);
/* Feature rows in use / reserved on the device (one row = 92 bytes over four arrays).  Since ABI 6000. */
int msorb_kf_store_rows(const msorb_kf_store* s, size_t* rows_in_use, size_t* rows_reserved);

/* msorb_search_by_bow with resident KeyFrames: kf1 = the query KeyFrame, kf2 = the train KeyFrame (KeyFrame-KeyFrame forms,
 * ORBmatcher.cc:872-1166) or -1 = the frame passed to the call (SearchByBoW(pKF, F, ...), :223-421; then every pair of the
 * call has kf2 == -1).  valid1 / avail2 / match12 / match21 / nmatches as in msorb_bow_pair. */
typedef struct msorb_bow_kf_pair {
    int kf1, kf2;
    const uint8_t *valid1, *avail2;
    int *match12, *match21;
    int nmatches;
} msorb_bow_kf_pair;
typedef struct msorb_bow_frame {  /* F.mDescriptors, F.mFeatVec as CSR, F.mvKeysUn[i].angle */
    int n;
    const uint8_t* desc;
    int fv_nodes;
    const int *fv_node, *fv_begin, *fv_feat;
    const float* angle;
} msorb_bow_frame;
int msorb_search_by_bow_kf(msorb_kf_store* s, msorb_bow_kf_pair* pairs, int n_pairs, const msorb_bow_frame* frame, int th_low,
                           int inclusive, float nnratio, int check_orientation, float* elapsed_ms);

/* msorb_search_for_triangulation with resident KeyFrames (fields as in msorb_triangulation_pair). */
typedef struct msorb_triangulation_kf_pair {
    int kf1, kf2;
    const uint8_t *valid1, *avail2, *stereo1, *stereo2;
    float F12[9];
    float ep[2];
    int* match12;
    int nmatches;
} msorb_triangulation_kf_pair;
int msorb_search_for_triangulation_kf(msorb_kf_store* s, msorb_triangulation_kf_pair* pairs, int n_pairs, int coarse,
                                      int check_orientation, float* elapsed_ms);

/* The neighbour loop of LocalMapping::CreateNewMapPoints (LocalMapping.cc:460-731) for resident pinhole KeyFrames without a second
 * camera: per neighbour, in the caller's order, SearchForTriangulation (:492), then for every matched pair the parallax test,
 * GeometricTools::Triangulate or KeyFrame::UnprojectStereo, the depth tests, the reprojection gates and the scale-consistency gate
 * (:578-712) — one upload, three small launches per neighbour on one stream, one read-back.  A query that got a point at neighbour i
 * is no query of neighbour i+1 (mpCurrentKeyFrame->AddMapPoint, :722 -> ORBmatcher.cc:1237-1241), which also frees the train it
 * would have claimed there: the result is the sequential loop's, not that of one msorb_search_for_triangulation_kf batch over all
 * neighbours.  Appended to ABI 6002 as the local bundle adjustment was: MSORB_ABI_VERSION stays 6002.
 *   geometry      Tcw = GetPose().matrix3x4() row major, Ow = GetCameraCenter(), fx .. mbf the KeyFrame's members,
 *                 u_right[n] = GetuRight(i) (stereo when >= 0), depth[n] = GetDepth(i)
 *   call          kf1 = mpCurrentKeyFrame; valid1[n1]: 1 = the feature has no map point now (bOnlyStereo = false);
 *                 coarse = bCoarse (:490); inertial = mbInertial (the 0.9996 / 0.9998 bound of :604);
 *                 th_far = mThFarPoints, <= 0 when mbFarPoints is off
 *   neighbour     kf2 and avail2[n2] (1 = no map point), its geometry, F12 / ep as in msorb_triangulation_pair.  The caller has
 *                 dropped the neighbours that fail the baseline test (:469-486).
 *   outputs       match12[n1]: vMatchedIndices after the orientation filter, for the masks at that point of the loop;
 *                 status[n1]: MSORB_NP_*; x3D[3 * n1]: the new point where the status is one of the three CREATED codes, 0 elsewhere;
 *                 nmatches; n_created.  The points of neighbour k, in ascending feature index, are the reference's creation order.
 * ratioFactor is 1.5f * mvScaleFactors[1] of kf1 (:454); mvLevelSigma2 / mvScaleFactors are the store's.  The arithmetic is float,
 * one rounded operation per reference operator (csrc/new_points_device.h); the singular vector of Triangulate comes from a restated
 * Jacobi SVD whose bit parity with a compiled Eigen is not pinned, and cos(2 atan2(mb/2, depth)) is evaluated as a rational
 * expression in double.  Not covered: KeyFrames with mpCamera2 (:526-576), fisheye models.
 * MSORB_E_INVALID, before anything is launched: unknown id, kf2 == kf1, a kf2 listed twice, a null required array, a KeyFrame with
 * more than 64 pyramid levels.  n_nb == 0 is MSORB_OK.  Thread-safe as the resident searches are. */
enum {
    MSORB_NP_NONE = 0,           /* not matched */
    MSORB_NP_TRIANGULATED = 1,   /* created (:606) */
    MSORB_NP_STEREO1 = 2,        /* created from kf1's stereo measurement (:614) */
    MSORB_NP_STEREO2 = 3,        /* created from kf2's stereo measurement (:620) */
    MSORB_NP_LOW_PARALLAX = 4,   /* :624 */
    MSORB_NP_NULL_W = 5,         /* :607, x3Dh(3) == 0 */
    MSORB_NP_STEREO_DEPTH = 6,   /* :630, UnprojectStereo with depth <= 0 */
    MSORB_NP_BEHIND1 = 7,        /* :635 */
    MSORB_NP_BEHIND2 = 8,        /* :639 */
    MSORB_NP_REPROJ1 = 9,        /* :654 / :666 */
    MSORB_NP_REPROJ2 = 10,       /* :680 / :691 */
    MSORB_NP_ZERO_DIST = 11,     /* :702 */
    MSORB_NP_FAR = 12,           /* :705 */
    MSORB_NP_SCALE_RATIO = 13    /* :711 */
};
typedef struct msorb_new_points_geometry {
    float Tcw[12];
    float Ow[3];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
    const float *u_right, *depth;
} msorb_new_points_geometry;
typedef struct msorb_new_points_call {
    int kf1;
    const uint8_t* valid1;
    msorb_new_points_geometry g1;
    int coarse, check_orientation, inertial;
    float th_far;
} msorb_new_points_call;
typedef struct msorb_new_points_neighbour {
    int kf2;
    const uint8_t* avail2;
    msorb_new_points_geometry g2;
    float F12[9];
    float ep[2];
    int* match12;
    uint8_t* status;
    float* x3D;
    int nmatches, n_created;
} msorb_new_points_neighbour;
int msorb_create_new_map_points_kf(msorb_kf_store* s, const msorb_new_points_call* call, msorb_new_points_neighbour* nb, int n_nb,
                                   float* elapsed_ms);
/* For measurements: with MSORB_NEW_POINTS_STAGES=1 in the environment (read once per process) a call that asks for elapsed_ms
 * brackets every launch with events; ms[0..2] = the calling thread's last call, summed over its neighbours: match, histogram,
 * new points. */
int msorb_create_new_map_points_stage_ms(float ms[3]);

/* KeyFrameDatabase on the device (src/KeyFrameDatabase.cc; the BowVectors are msorb_bow_transform's).  Appended to ABI 6002:
 * MSORB_ABI_VERSION is unchanged, so a caller that needs these entries asks the loader for them (a library built before them
 * reports 6002 as well).
 * An entry is one KeyFrame's BowVector: word ids strictly ascending and < n_words (= the vocabulary's size, the length of the
 * reference's mvInvertedFile, :35), values as doubles.  The database keeps them on one device as a forward file, plus per
 * entry its add sequence number: one `add` appends the KeyFrame to all the lists of the reference's inverted file at once
 * (:39-45), so the order of two KeyFrames inside any list is their add order, and an erase followed by an add moves a
 * KeyFrame to the back.  Thread-safe: queries may run concurrently with each other; add / erase / clear wait for running
 * queries.  There is no CPU fallback: without a device msorb_kf_database_create returns MSORB_E_NO_DEVICE. */
typedef struct msorb_kf_database msorb_kf_database;
int msorb_kf_database_create(int device, int n_words, msorb_kf_database** out);
void msorb_kf_database_destroy(msorb_kf_database* db);
/* KeyFrameDatabase::add (:39-45).  *entry_id identifies the entry in later calls; ids of erased entries are handed out again.
 * Unsorted / repeated / out-of-range words: MSORB_E_INVALID, the database is unchanged.  n == 0 is an entry no query meets. */
int msorb_kf_database_add(msorb_kf_database* db, const int* word, const double* value, int n, int* entry_id);
/* KeyFrameDatabase::erase (:47-66): removes exactly what the add entered (the reference walks the KeyFrame's CURRENT
 * BowVector, which in MS-SLAM is the one it was added with).  The rows and the id go to the next add (first fit). */
int msorb_kf_database_erase(msorb_kf_database* db, int entry_id);
/* KeyFrameDatabase::clear (:68-72).  Every id is invalid afterwards; the device arrays stay reserved. */
int msorb_kf_database_clear(msorb_kf_database* db);
/* Live entries, the bound of the ids handed out so far (ids are < id_bound), BowVector elements in use / reserved on the
 * device (12 bytes each over two arrays).  Any output may be NULL. */
int msorb_kf_database_info(const msorb_kf_database* db, int* n_entries, int* id_bound, size_t* rows_in_use, size_t* rows_reserved);
/* The place-recognition query up to the scores: DetectRelocalizationCandidates :746-792 (rule 0) and MS-SLAM's
 * DetectNBestCandidates :612-668 (rule 1), with the L1 score of Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68.
 * word / value [n]: the query BowVector (v1 of the score).  listed [id_bound] (NULL = all): which entries the reference's
 * walk would put on lKFsSharingWords (rule 0: mnRelocQuery != F->mnId, :753; rule 1: mnPlaceRecognitionQuery != pKF->mnId &&
 * mbSparsified && !spConnectedKF.count(pKFi), :620-625) - members of the caller's KeyFrames, so the caller builds the mask.
 * Reported are all live entries sharing at least one word with the query, *n_sharing of them:
 *   [0, *n_listed)          the listed ones in the order of lKFsSharingWords (first encounter of a walk over the query's words
 *                           ascending and each word's list front to back = ordered by smallest common word, then add order), each
 *                           with common_words (mnRelocWords / mnPlaceRecognitionWords, the size of the word intersection) and
 *                           score = the DOUBLE ScoringObject.cpp:65 returns, its additions made in ascending word order as the merge
 *                           walk makes them (the reference narrows it to float si, :663 / :788).  Every listed entry is scored; the
 *                           reference scores those with common_words > *min_common_words (:660, :785), which the caller applies;
 *   [*n_listed, *n_sharing) the others in ascending id, with common_words and score 0 (the reference touches their word counters
 *                           too, :622 / :631 / :759).
 * *max_common_words: the largest common_words of the listed entries (:639-644, :767-772); *min_common_words: max * 0.8f for
 * rule 0 (:774), max > 10 ? max * 0.8f : max * 0.6f for rule 1 (:646-650), int * float truncated as there.  Both 0 without a
 * listed entry.  capacity = length of entry / common_words / score; *n_sharing > capacity: MSORB_E_CAPACITY with *n_sharing
 * set and nothing else written (id_bound always suffices).  *elapsed_ms (may be NULL) = device time of the kernel. */
int msorb_kf_database_query(msorb_kf_database* db, const int* word, const double* value, int n, const uint8_t* listed, int rule,
                            int* entry, int* common_words, double* score, int capacity, int* n_sharing, int* n_listed,
                            int* max_common_words, int* min_common_words, float* elapsed_ms);

/* Optimizer::PoseOptimization (src/Optimizer.cc:759-1037) for pinhole mono / stereo frames on the device: the four rounds, every
 * Levenberg step and trial of g2o (core/optimization_algorithm_levenberg.cpp:61-170) and the classification after each round in
 * ONE launch, in double.  Appended to ABI 6002 as the KeyFrame database was: MSORB_ABI_VERSION stays 6002, so a caller that
 * needs these entries asks the loader for them.  The two-camera arm (:870-931) has its own entry at the end of this header
 * (msorb_pose_optimization_rig_batch); the inertial variants are not covered here.
 * An observation is a stereo edge when its u_right >= 0 (:808) and a mono edge otherwise.  Two calls on the same input return
 * the same bits.  Re-entrant: every calling thread has its own stream and staging. */
typedef struct msorb_pose_problem {      /* one Optimizer::PoseOptimization call */
    float q[4], t[3];                    /* pFrame->GetPose(): unit quaternion x,y,z,w + translation */
    float fx, fy, cx, cy, mbf;
    int n;                               /* observations */
} msorb_pose_problem;
typedef struct msorb_pose_result {
    float q[4], t[3];                    /* what SetPose receives (:1033-1035) */
    double qd[4], td[3];                 /* the double estimate before the narrowing */
    int n_initial, n_bad;                /* return value = n_initial - n_bad */
    int iterations[4], rejected_trials[4];   /* per round: solve() calls made, trials popped; -1 = round not run */
} msorb_pose_result;
/* Observations up to which a problem is held in registers; a larger one walks global memory (same additions, same result). */
int msorb_pose_optimization_capacity(void);
/* n_problems independent calls (the relocalisation candidates, :3746-3777 of Tracking.cc) as flat host arrays: one upload, one
 * launch, one read-back.  Problem i owns the observations [obs_offset[i], obs_offset[i+1]) (obs_offset[0] = 0, the difference =
 * problems[i].n) of xy [2 per observation: kpUn.pt], u_right, inv_sigma2 (already mvInvLevelSigma2[octave]) and pos_w [3 per
 * observation: pMP->GetWorldPos()].  Entries the reference skips (no map point, isBad()) are simply not passed.
 * outlier_out [per observation] = mvbOutlier after the last round.  With n < 3 the reference returns 0 before it touches the
 * pose (:936-937): q / t repeat the input, the flags are cleared, n_bad = n_initial and every round reads -1.
 * *elapsed_ms (may be NULL) = device time of the kernel. */
int msorb_pose_optimization_batch(int device, int n_problems, const msorb_pose_problem* problems, const int* obs_offset,
                                  const float* xy, const float* u_right, const float* inv_sigma2, const float* pos_w,
                                  uint8_t* outlier_out, msorb_pose_result* results, float* elapsed_ms);
/* The frame form: x, y, u_right and the octave are read from the keypoint table resident on the handle, which holds mvKeysUn
 * only when mvKeysUn == mvKeys, i.e. for rectified input.  has_point [N] marks the keypoints with a usable map point, pos_w
 * [3 N] their world positions (read where has_point is set), inv_level_sigma2 [nlevels] = mvInvLevelSigma2; p->n is ignored.
 * Only the indices of the marked keypoints and their positions go up.  outlier [N] is written where has_point is set and left
 * alone elsewhere.  The result equals msorb_pose_optimization_batch on the same data bit for bit. */
int msorb_frame_pose_optimization(msorb_frame* f, const msorb_pose_problem* p, const uint8_t* has_point, const float* pos_w,
                                  const float* inv_level_sigma2, int nlevels, uint8_t* outlier, msorb_pose_result* r);

/* Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1040-1407) for pinhole KeyFrames without a second camera on the device:
 * g2o's Levenberg-Marquardt over the KeyFrame poses and the map points (optimization_algorithm_levenberg.cpp:61-170 under
 * sparse_optimizer.cpp:376-389), the points eliminated by the Schur complement (block_solver.hpp:354-486), in double, and the
 * classification of :1331-1373.  Appended to ABI 6002 as the pose optimisation was: MSORB_ABI_VERSION stays 6002.  Not covered:
 * the EdgeSE3ProjectXYZToBody arm (:1281-1317) and an inertial map (setUserLambdaInit, :1113); the caller keeps the reference's
 * routine for those.  Two calls on the same input return the same bits.  Re-entrant: every calling thread has its own stream and
 * staging. */
#define MSORB_E_ARG MSORB_E_INVALID      /* an index out of range, edges that are not point-major, a missing array */
typedef struct msorb_ba_keyframe { float q[4], t[3]; float fx, fy, cx, cy, mbf; int fixed; } msorb_ba_keyframe;
typedef struct msorb_ba_result {
    int status;             /* 0 optimised; 1 no fixed KeyFrame: nothing touched (:1098-1102); 2 stop flag set before the first iteration (:1323-1325): nothing touched */
    int iterations;         /* solve() calls made (optimize's return value) */
    int trials, rejected_trials;
    int n_outliers;
    double chi2_initial, chi2_final, lambda_final;
} msorb_ba_result;
/* The largest number of free (not fixed) KeyFrames a call accepts: the reduced system is solved densely by one workgroup.
 * More: MSORB_E_CAPACITY, nothing launched.  Points and edges are bounded by device memory only. */
int msorb_local_ba_capacity(void);
/* kfs [n_kf]: GetPose() as unit quaternion x,y,z,w + translation, the camera, fixed != 0 for lFixedCameras and the InitKFid
 * KeyFrame (:1136, :1152).  pos_w [3 per point].  Edges are point-major (all edges of point 0, then of point 1, ...: the order
 * in which :1196-1320 makes them): edge_kf, edge_point, xy [2 per edge: kpUn.pt], u_right (>= 0 marks a stereo edge, :1246),
 * inv_sigma2 (mvInvLevelSigma2[octave]).  max_iterations: the reference passes 10.  *stop_flag (may be NULL) is read where g2o
 * calls terminate(): before every iteration and between the trials of one.  Outputs: kf_qt_out [7 per KeyFrame] the narrowed
 * estimate that SetPose receives (:1393; a fixed KeyFrame's repeats its input), pos_out [3 per point] (:1402), kf_qt_d / pos_d
 * (may be NULL) the doubles before the narrowing, edge_outlier [per edge] 1 where chi2 > 5.991 (mono) / 7.815 (stereo) or the
 * depth is not positive at the final estimate: the pairs of vToErase.  With status 1 or 2 the outputs repeat the inputs and no
 * flag is set.  Without an edge there is nothing to optimise: status 0, zero iterations.  MSORB_E_ARG: an index out of range or
 * edges that are not point-major.  *elapsed_ms (may be NULL) = device time from the first launch to the classification. */
int msorb_local_ba(int device, int n_kf, const msorb_ba_keyframe* kfs, int n_points, const float* pos_w,
                   int n_edges, const int* edge_kf, const int* edge_point, const float* xy, const float* u_right,
                   const float* inv_sigma2, int max_iterations, const volatile int* stop_flag,
                   float* kf_qt_out, double* kf_qt_d, float* pos_out, double* pos_d, uint8_t* edge_outlier, msorb_ba_result* r,
                   float* elapsed_ms);
/* For measurements: with MSORB_LOCAL_BA_STAGES=1 in the environment (read once per process) every msorb_local_ba call brackets
 * its stages with events, and this returns the device ms of the calling thread's last call spent in: [0] the linearisations
 * (errors, Jacobians, the per-vertex sums), [1] the Schur complements, [2] the dense solves, [3] the rest of the trials (update,
 * errors, cost).  Without the variable: MSORB_E_ARG, zeros. */
int msorb_local_ba_stage_ms(float ms[4]);

/* Optimizer::BundleAdjustment (src/Optimizer.cc:60-364, the body of GlobalBundleAdjustemnt) for pinhole KeyFrames without a second
 * camera on the device: the global bundle adjustment of the monocular initialisation (Tracking.cc:2561) and of loop closing
 * (LoopClosing.cc:2228).  Appended to ABI 6002 as the local bundle adjustment was: MSORB_ABI_VERSION stays 6002.  The arrays and
 * the point-major edge order are msorb_local_ba's; what differs restates the reference: fixed marks mnId == GetInitKFid() (:122);
 * no fixed KeyFrame is nothing special (no status 1); robust == 0 leaves the Huber kernel off (:174, :206); optimize(n_iterations)
 * runs once and nothing is classified (n_outliers is 0); a stop flag that is already set yields zero iterations (no status 2);
 * a point without an edge is no vertex (:261-263): point_included [per point] is 0 and its pos_out repeats the input.  The
 * reduced system is solved by a blocked, multi-workgroup L D L^T (below).  More free KeyFrames than the capacity, or no room on
 * the device for the reduced system: MSORB_E_CAPACITY, nothing launched, no output written.  Two calls on the same input return
 * the same bits.  Re-entrant like msorb_local_ba. */
int msorb_bundle_adjustment_capacity(void);            /* free KeyFrames: 1024 (the reduced system is 6144^2 doubles = 302 MB) */
int msorb_bundle_adjustment(int device, int n_kf, const msorb_ba_keyframe* kfs, int n_points, const float* pos_w,
                            int n_edges, const int* edge_kf, const int* edge_point, const float* xy, const float* u_right,
                            const float* inv_sigma2, int n_iterations, int robust, const volatile int* stop_flag,
                            float* kf_qt_out, double* kf_qt_d, float* pos_out, double* pos_d, uint8_t* point_included,
                            msorb_ba_result* r, float* elapsed_ms);
/* msorb_local_ba_stage_ms for the calling thread's last msorb_bundle_adjustment call (the same environment variable). */
int msorb_bundle_adjustment_stage_ms(float ms[4]);
/* The dense solver of msorb_bundle_adjustment alone: S x = b for a symmetric S by L D L^T without pivoting and without a square
 * root, right-looking and blocked: a panel of *panel columns is factored by one workgroup in LDS, the rows below it and the
 * trailing lower triangle (in tiles of *tile) by as many workgroups as there are rows and tiles.  Every entry goes through the
 * subtractions of the column-by-column factorisation in the same order, so two runs, and any panel width, return the same bits. */
int msorb_ldlt_block_sizes(int* panel, int* tile);
/* S: n x n doubles, row-major, the lower triangle is read; b, x: n; any n >= 1.  Host arrays: upload, solve, read-back.
 * *ok = 0: a pivot was not positive ("solver failed"), x untouched.  *elapsed_ms (may be NULL): device time of the solve. */
int msorb_ldlt_solve(int device, int n, const double* S, const double* b, double* x, int* ok, float* elapsed_ms);

/* Sim3Solver's RANSAC (src/Sim3Solver.cc:228-373) for two pinhole cameras on the device, every hypothesis at once.  Appended to ABI
 * 6002 as the local bundle adjustment was: MSORB_ABI_VERSION stays 6002.  The draws of :254-265 do not depend on the data, so the
 * caller draws the minimal sets of all iterations beforehand (DUtils::Random::RandomInt with the swap-with-back rule of :256-264)
 * and hands them in as index triples; ComputeSim3 (:390-491) and CheckInliers (:494-518) then run for all of them in one launch, and
 * a second launch applies the loop's sequential rule (:344-366) to the counts in hypothesis order: starting from best_inliers_in
 * (mnBestInliers), a hypothesis replaces the running best when count >= best, and the scan stops at the first one where that holds
 * and count > min_inliers (mRansacMinInliers).
 *   problem   n correspondences, n_hyp triples, fix_scale = mbFixScale, cam1 / cam2 = fx, fy, cx, cy of pCamera1 / pCamera2
 *             (Pinhole only)
 *   result    winner: the hypothesis the loop ends on or, not converged, the last one that replaced the best (-1: none reached
 *             best_inliers_in; the record is then all zero); converged: the stop above happened (bConverge); consumed: the
 *             iterations the loop went through (mnIterations advances by it: winner + 1 when converged, n_hyp otherwise);
 *             n_inliers = mnInliersi, s = ms12i, R = mR12i (row major), t = mt12i, T12 = mT12i (row major) of the winner
 * Problem i owns the correspondences [corr_offset[i], corr_offset[i+1]) of X1 / X2 (3 floats each: mvX3Dc1 / mvX3Dc2) and max_err1 /
 * max_err2 (mvnMaxError1 / mvnMaxError2, which the reference holds as integers, Sim3Solver.h:85-86: the caller passes the truncated
 * values as floats) and the hypotheses [hyp_offset[i], hyp_offset[i+1]) of triples (3 indices into the problem's own
 * correspondences); both offset arrays start at 0 and advance by n / n_hyp.  inlier_out [per correspondence] = the winner's
 * mvbInliersi (0 without a winner); counts_out [per hypothesis] (may be NULL) = every hypothesis' mnInliersi, also of those behind a
 * converged winner.  The arithmetic is float, one rounded operation per reference operator (csrc/sim3_device.h); the eigenvector
 * of :432-441 comes from a cyclic Jacobi iteration and the rotation of :441-447 from that quaternion in algebraic form, so bit
 * parity with a compiled Eigen / libm is not pinned.  Non-finite results are results: a degenerate triple
 * gives a NaN transform with no inliers and takes part in the >= rule as in the reference.
 * MSORB_E_INVALID, before anything is launched and with every output untouched: n < 3, n_hyp < 1, offsets that do not match, an
 * index of a triple that is negative, >= n or repeated, a null required array.  n_problems == 0 is MSORB_OK.  Flat host arrays,
 * one upload, two launches, one read-back.  Two calls on the same input return the same bits, and a batch returns the bits of
 * the single calls.  Re-entrant: every calling thread has its own stream and staging.  *elapsed_ms (may be NULL) = device time
 * of the two launches. */
typedef struct msorb_sim3_problem {
    int n, n_hyp, fix_scale, min_inliers, best_inliers_in;
    float cam1[4], cam2[4];
} msorb_sim3_problem;
typedef struct msorb_sim3_result {
    int winner, converged, consumed, n_inliers;
    float s, R[9], t[3], T12[16];
} msorb_sim3_result;
int msorb_sim3_ransac_batch(int device, int n_problems, const msorb_sim3_problem* problems, const int* corr_offset,
                            const int* hyp_offset, const float* X1, const float* X2, const float* max_err1, const float* max_err2,
                            const int* triples, uint8_t* inlier_out, int* counts_out, msorb_sim3_result* results, float* elapsed_ms);

/* Optimizer::OptimizeSim3 (src/Optimizer.cc:1986-2242 and :2244-2429) for two pinhole cameras on the device, after the gathering
 * loops: the 7-DoF Sim3 vertex over the EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ pair of every correspondence, g2o's
 * Levenberg loop and both classifications in ONE launch, in double.  Appended to ABI 6002 as the Sim3 RANSAC was:
 * MSORB_ABI_VERSION stays 6002.  This fork comments linearizeOplus out on both edges (OptimizableTypes.h:192,213), so g2o
 * differentiates numerically (core/base_binary_edge.hpp:131-205, central differences, delta = 1e-9, through oplus); the device
 * does the same.  The routine: optimize(its[0]) with Huber (delta = (float)sqrt(th2)) over all pairs, run whenever n >= 1; the
 * first classification reads the chi2 the last trial left and drops a pair when either chi2 > th2 (n_bad of them), the others
 * lose the kernel; with n - n_bad < min_pairs the reference returns 0 before it writes g2oS12: status 1, n_in 0, the estimate
 * repeats the input, the flags are those of the first classification; otherwise optimize(n_bad > 0 ? its[1] : its[2]) (a fresh
 * run), computeError of the survivors at the final estimate and the final classification: status 0, n_in = the survivors that
 * pass, the estimate in double.  The reference passes its = {5, 10, 5} and min_pairs = 10 (:2211) or 5 (:2397).
 * Nothing normalises the quaternion (g2o::Sim3 does not).  Non-finite results are results: a point with z <= 0 after a map
 * gives an infinite or negative projection and takes part as in the reference. */
typedef struct msorb_sim3_opt_problem {
    double q[4], t[3], s;               /* g2oS12: rotation x, y, z, w, translation, scale */
    float cam1[4], cam2[4];             /* fx, fy, cx, cy of pKF1->mpCamera / pKF2->mpCamera (Pinhole only) */
    float th2;
    int fix_scale;                      /* bFixScale */
    int min_pairs;
    int its[3];                         /* each >= 1 */
    int n;                              /* pairs */
    int reserved;                       /* 0 */
} msorb_sim3_opt_problem;
typedef struct msorb_sim3_opt_result {
    double q[4], t[3], s;               /* the estimate; the input again with status 1 */
    int status;                         /* 0 optimised; 1 fewer than min_pairs pairs left after the first classification */
    int n_pairs, n_bad, n_in;           /* nCorrespondences, nBad, the return value */
    int iterations[2], rejected_trials[2];   /* per optimize() call: solve() calls made, trials popped; -1 = not run */
} msorb_sim3_opt_result;
/* Pairs up to which a problem is held in registers; a larger one walks global memory (same additions, same result). */
int msorb_sim3_optimization_capacity(void);
/* n_problems independent calls as flat host arrays: one upload, one launch, one read-back.  Problem i owns the pairs
 * [pair_offset[i], pair_offset[i+1]) (pair_offset[0] = 0, the difference = problems[i].n) of P1c / P2c (3 floats per pair: the
 * floats R1w*P3D1w + t1w and R2w*P3D2w + t2w that the reference casts to double), obs1 / obs2 (2 floats per pair) and
 * inv_sigma2_1 / inv_sigma2_2.  bad_out [per pair]: 0 kept, 1 bad at the first classification, 2 bad at the final one;
 * chi2_out [2 doubles per pair: e12, e21] (may be NULL) = what the last classification a pair took part in read.
 * MSORB_E_INVALID, before anything is launched and with every output untouched: a null required array, offsets that do not match,
 * n < 0, an entry of its below 1.  n_problems == 0 is MSORB_OK.  Two calls on the same input return the same bits, and a batch
 * returns the bits of the single calls.  Re-entrant: every calling thread has its own stream and staging.  *elapsed_ms (may be
 * NULL) = device time of the kernel. */
int msorb_sim3_optimization_batch(int device, int n_problems, const msorb_sim3_opt_problem* problems, const int* pair_offset,
                                  const float* P1c, const float* P2c, const float* obs1, const float* obs2,
                                  const float* inv_sigma2_1, const float* inv_sigma2_2, uint8_t* bad_out, double* chi2_out,
                                  msorb_sim3_opt_result* results, float* elapsed_ms);

/* Frame::ComputeStereoMatches (Frame.cc:743-913, median rejection :899-912 included) for every stereo pair of the last
 * msorb_extract_batch() call of `h`, all on the device: pair p = images 2p (left) and 2p+1 (right) of that batch.
 * d_keypoints / d_descriptors / capacity are the arrays that call filled, d_counts[2*n_pairs] the keypoint counts as a
 * DEVICE array.  Outputs (device): d_u_right / d_depth [n_pairs][capacity] (mvuRight / mvDepth of the left image, -1 =
 * none; entries past the left count are not written), d_n_oob[n_pairs] (may be NULL; see msorb_stereo_matches).
 * The pyramids of the batch must still be alive (no other extract call on `h` in between).  *elapsed_ms (may be NULL) =
 * device time of the two kernels. */
int msorb_stereo_matches_batch(msorb_extractor* h, int n_pairs, const msorb_keypoint* d_keypoints,
                               const uint8_t* d_descriptors, int capacity, const int* d_counts, int max_left, float mb,
                               float mbf, float* d_u_right, float* d_depth, int* d_n_oob, float* elapsed_ms);

/* The same with the two eyes in separate batches: left images = the last msorb_extract_batch() of `left`, right images = the
 * last msorb_extract_batch() or msorb_pyramid_batch() of `right` (both handles on ONE device; pair p = image p of each).
 * The right keypoints / descriptors / counts may have been extracted on another device and gathered (RCCL / peer copy). */
int msorb_stereo_matches_split(msorb_extractor* left, msorb_extractor* right, int n_pairs, const msorb_keypoint* d_kps_left,
                               const uint8_t* d_desc_left, const int* d_counts_left, const msorb_keypoint* d_kps_right,
                               const uint8_t* d_desc_right, const int* d_counts_right, int capacity, int max_left, float mb,
                               float mbf, float* d_u_right, float* d_depth, int* d_n_oob, float* elapsed_ms);

/* ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:2277-2318) on histogram bin sizes; ind[3]. Host only. */
int msorb_three_maxima(const int* bin_sizes, int n_bins, int* ind);

/* ------------------------------------------------------------------------------------------------
 * Map sparsification — constraint-matrix assembly of MapSparsification::Sparsifying
 * (src/MapSparsification.cc:58-151) as CSR, built on the device.  The caller flattens, under the
 * reference's locks, what the loop reads:
 *   window keyframe k (vpKFs order) owns slots [kf_slot_begin[k], kf_slot_begin[k+1]) in the grid walk
 *   order of :82-84 (grid column, grid row, cell index list): slot_point = map point id or -1 (null or
 *   isBad()), slot_cell = column*rows+row;  point_nobs = Observations(); obs_begin/obs_kf = GetObservations()
 *   keyframe ids per point; kf_in_window = (mnMapSaprsificationId == mnId); kf_num_mps = GetNumberMPs().
 * Outputs (host arrays): columns = map points in first-encounter order (col_point, obj_coef = nMaxObs -
 * Observations()); rows in the order the reference adds constraints: per window keyframe its valid cells
 * (row_kind 0, rhs 1) then the keyframe row (kind 1, rhs N), then one row per outside keyframe observing a
 * column point (kind 2, rhs count/GetNumberMPs()*N) in ascending keyframe id (the reference walks a
 * std::map keyed by shared_ptr there, i.e. run-dependent order).  row_begin has *n_rows+1 entries; col_idx
 * lists column indices in the order the reference accumulates the terms.  Every row owns one implicit slack
 * variable (th_grid: binary, cost GridLambda; th: integer 0..1000, cost Lambda) — see INTEGRATION.md for the
 * GUROBI C-API mapping.  n_max_obs_floor: max Observations() over map points of window keyframes that are in
 * no grid cell (normally 0).
 * The caller's contract for obs_kf: the list of a point holds a keyframe id AT MOST ONCE, as the reference's
 * std::map<KeyFrame, ...> of GetObservations() does.  It is not checked.  An id listed twice would be counted
 * twice in the row's rhs and appear once in col_idx (one bit per column in the row's bitmap), so that
 * row_begin and col_idx disagree.  A point MAY sit in several slots of one keyframe or cell: its column opens
 * once and every slot is a term of the cell row and of the keyframe row, as :100-107 add them.
 * ---------------------------------------------------------------------------------------------- */
int msorb_visibility_csr(int device, int n_window_kf, const int* kf_slot_begin, const int* slot_point,
                         const int* slot_cell, int n_points, const int* point_nobs, const int* obs_begin,
                         const int* obs_kf, int n_kf_total, const uint8_t* kf_in_window, const int* kf_num_mps, int n,
                         int n_max_obs_floor, int* n_cols, int* col_point, int cap_cols, int* n_rows, int* row_begin,
                         int* row_kind, int* row_owner, float* row_rhs, int cap_rows, int* col_idx, int cap_nnz,
                         int* nnz, float* obj_coef, int* n_max_obs);

/* ------------------------------------------------------------------------------------------------
 * Bag of words — DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>::transform(features, BowVector&,
 * FeatureVector&, levelsup) (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1123-1191, descent :1218-1259) as
 * called by Frame::ComputeBoW (src/Frame.cc:670-677) and KeyFrame::ComputeBoW with levelsup = 4.
 * The vocabulary tree lives on the device (children of a node contiguous); the descent is one 16/32-lane
 * group per descriptor, the two std::map containers are assembled per frame by a sort + run-length pass
 * that repeats the reference's accumulation order (sequential double adds), so values are bit-identical.
 * ---------------------------------------------------------------------------------------------- */
typedef struct msorb_vocabulary msorb_vocabulary;

/* Tree as loadFromTextFile (TemplatedVocabulary.h:1338-1423) builds it: n_nodes nodes, node 0 = root;
 * for i >= 1: parent[i] (< i is not required), is_leaf[i] = the file's leaf flag (word ids are handed out to
 * flagged nodes in node order), descriptors[i*32..], weights[i].  scoring / weighting = the file header's
 * ScoringType / WeightingType (BowVector.h:39-56); ORBvoc.txt is k=10, L=6, L1_NORM(0), TF_IDF(0). */
int msorb_vocabulary_create(int device, int k, int L, int scoring, int weighting, int n_nodes, const int* parent,
                            const uint8_t* is_leaf, const uint8_t* descriptors, const double* weights,
                            msorb_vocabulary** out);
/* Reads the ORBvoc.txt text format (header "k L scoring weighting", then one line per node:
 * "parent is_leaf b0 .. b31 weight").  Empty lines are skipped (the reference's `while(!f.eof())` loop turns a
 * trailing newline into a phantom child of the root with an indeterminate descriptor; not reproduced). */
int msorb_vocabulary_load_text(int device, const char* path, msorb_vocabulary** out);
void msorb_vocabulary_destroy(msorb_vocabulary* v);
int msorb_vocabulary_info(const msorb_vocabulary* v, int* k, int* L, int* n_nodes, int* n_words);

/* transform() for n_frames frames whose descriptors are DEVICE resident (frame i: d_descriptors +
 * i*desc_stride*32, h_counts[i] rows — exactly msorb_extract_batch's outputs).  Device outputs, `stride` entries
 * per frame (stride >= max count, <= 8192): BowVector as ascending (d_bow_word, d_bow_value) with d_n_bow[i]
 * entries; FeatureVector as ascending node ids d_fv_node with CSR d_fv_begin (stride+1 per frame) into d_fv_feat
 * (feature indices, ascending inside a node) and d_n_fv[i] nodes.  elapsed_ms (may be NULL): kernel time. */
int msorb_bow_transform_batch(msorb_vocabulary* v, const uint8_t* d_descriptors, const int* h_counts, int n_frames,
                              int desc_stride, int levelsup, int stride, int* d_bow_word, double* d_bow_value,
                              int* d_n_bow, int* d_fv_node, int* d_fv_begin, int* d_fv_feat, int* d_n_fv,
                              float* elapsed_ms);
/* One frame, HOST arrays in and out (capacity n entries each, fv_begin n+1).  feat_word / feat_node /
 * feat_weight (may be NULL): per-feature result of the descent (:1218-1259). */
int msorb_bow_transform(msorb_vocabulary* v, const uint8_t* descriptors, int n, int levelsup, int* bow_word,
                        double* bow_value, int* n_bow, int* fv_node, int* fv_begin, int* fv_feat, int* n_fv,
                        int* feat_word, int* feat_node, double* feat_weight);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:351-429) batched over map points: point p owns the
 * descriptors [obs_begin[p], obs_begin[p+1]) of `descriptors` (32 B rows, in the order the reference collects
 * vDescriptors).  best_idx[p] = position inside the point's list of the descriptor with the least median
 * distance to the others (first minimum; -1 for a point without descriptors), best_median[p] (may be NULL) that
 * median.  Host arrays; elapsed_ms (may be NULL): kernel time. */
int msorb_distinctive_descriptors(int device, const uint8_t* descriptors, const int* obs_begin, int n_points,
                                  int* best_idx, int* best_median, float* elapsed_ms);

/* ------------------------------------------------------------------------------------------------
 * Frame::isInFrustum (src/Frame.cc:512-571, pinhole / Nleft == -1) over n map points — the pre-pass of
 * Tracking::SearchLocalPoints (src/Tracking.cc:3343-3361); its outputs are exactly the per-point arrays
 * msorb_search_by_projection_mps takes.  The caller skips nothing: points the reference does not visit
 * (mnLastFrameSeen == frame id, isBad()) are simply not passed.
 * ---------------------------------------------------------------------------------------------- */
typedef struct msorb_frustum {
    float Rcw[9];                       /* mRcw, row major */
    float tcw[3];                       /* mtcw */
    float Ow[3];                        /* mOw (camera centre) */
    float fx, fy, cx, cy;               /* Pinhole mvParameters[0..3] */
    float min_x, max_x, min_y, max_y;   /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    float mbf;                          /* baseline * fx */
    float log_scale_factor;             /* mfLogScaleFactor */
    int n_scale_levels;                 /* mnScaleLevels */
} msorb_frustum;

/* Inputs: pos_w / normal = GetWorldPos() / GetNormal() (3 floats per point), max_distance / min_distance =
 * mfMaxDistance / mfMinDistance (the 1.2 / 0.8 invariance factors are applied inside, MapPoint.cc:528-538).
 * Outputs (host, n entries): track_in_view = the return value / mbTrackInView; proj_x, proj_y = mTrackProjX/Y
 * (-1 when the point is behind the camera or outside the image, the projection otherwise, like :515-540);
 * proj_xr, track_depth, scale_level (PredictScale, MapPoint.cc:557-572), view_cos — written when in view, 0
 * otherwise (the reference leaves stale values there that no caller reads).  elapsed_ms may be NULL. */
int msorb_is_in_frustum(int device, const msorb_frustum* f, float viewing_cos_limit, int n, const float* pos_w,
                        const float* normal, const float* max_distance, const float* min_distance,
                        uint8_t* track_in_view, float* proj_x, float* proj_y, float* proj_xr, float* track_depth,
                        int* scale_level, float* view_cos, float* elapsed_ms);

/* ------------------------------------------------------------------------------------------------
 * The tracking front-end of one frame as ONE device-resident chain — BASELINE configs[2] ("extract +
 * SearchByProjection inside the full Tracking loop"), SURVEY.md 8f-2.  The extractor's outputs do not travel to the host and
 * back on their way into the matcher: Frame::AssignFeaturesToGrid (src/Frame.cc:385-416, PosInGrid :657-667) runs on the
 * device keypoints, Frame::isInFrustum writes the window queries of ORBmatcher::SearchByProjection on the device, and one
 * block comes back for the sequential claim replay.
 * ---------------------------------------------------------------------------------------------- */

/* msorb_frame_set from DEVICE arrays (e.g. the outputs of msorb_extract_batch): keypoints (cv::KeyPoint layout), 32-byte
 * descriptors, mvuRight (NULL = all -1), on the frame's device.  The grid is built by a device counting sort that keeps the
 * ascending keypoint index inside a cell (the reference's push_back order, Frame.cc:405-414). */
int msorb_frame_set_device(msorb_frame* f, const msorb_keypoint* d_keypoints, int n, const uint8_t* d_descriptors,
                           const float* d_u_right, float min_x, float max_x, float min_y, float max_y,
                           const float* scale_factors, int nlevels);

/* Inspection: mGrid of the frame as CSR — cell_begin[64*48 + 1] (cell = ix*48 + iy = mGrid[ix][iy]), cell_idx[*n_assigned]
 * keypoint indices in the reference's insertion order. */
int msorb_frame_grid(msorb_frame* f, int* cell_begin, int* cell_idx, int capacity, int* n_assigned);

/* Frame::Frame(imLeft, imRight, ...) up to and including AssignFeaturesToGrid (Frame.cc:119-137, :385-416): msorb_extract_stereo
 * (same arguments, same host outputs) and, on the same stream before the one synchronisation, the frame handle `f` is filled
 * from the device-resident left keypoints / descriptors / mvuRight.  min_x .. max_y = mnMinX .. mnMaxY (rectified: 0, cols, 0,
 * rows).  `h` and `f` must live on one device.  Afterwards `f` serves every msorb_search_* entry like a frame loaded with
 * msorb_frame_set. */
int msorb_extract_stereo_frame(msorb_extractor* h, msorb_frame* f, const uint8_t* left, const uint8_t* right, int rows, int cols,
                               size_t stride_left, size_t stride_right, float mb, float mbf, msorb_keypoint* kps_left,
                               uint8_t* desc_left, int* n_left, msorb_keypoint* kps_right, uint8_t* desc_right, int* n_right,
                               int capacity, float* u_right, float* depth, int* n_oob, float min_x, float max_x, float min_y,
                               float max_y);

/* Tracking::SearchLocalPoints from its second loop on (src/Tracking.cc:3343-3388): Frame::isInFrustum(pMP, viewing_cos_limit)
 * for the m local map points (Frame.cc:512-571; inputs as msorb_is_in_frustum; visit[i] = the loop reaches the point: not
 * mnLastFrameSeen == mnId, not isBad(); NULL = all) and ORBmatcher(nnratio).SearchByProjection(F, mvpLocalMapPoints, th,
 * bFarPoints, thFarPoints) (ORBmatcher.cc:43-142; bad / sparsified / mp_desc / obs / frame_mp as msorb_search_by_projection_mps)
 * as one chain on the device: one upload, frustum + window queries, window search, one read-back, then the claim replay.
 * Outputs: the per-point scratch of isInFrustum (any may be NULL) and frame_mp / *nmatches.  Results are identical to
 * msorb_is_in_frustum followed by msorb_search_by_projection_mps. */
int msorb_search_local_points(msorb_frame* f, const msorb_frustum* frustum, float viewing_cos_limit, int m, const float* pos_w,
                              const float* normal, const float* max_distance, const float* min_distance, const uint8_t* visit,
                              const uint8_t* bad, const uint8_t* sparsified, const uint8_t* mp_desc, const int* obs, int* frame_mp,
                              float th, int far_points, float th_far_points, float nnratio, uint8_t* track_in_view, float* proj_x,
                              float* proj_y, float* proj_xr, float* track_depth, int* scale_level, float* view_cos, int* nmatches);

/* msorb_extract_stereo_frame + msorb_search_local_points in ONE call with ONE synchronisation, for a caller that knows the
 * pose before the images arrive (motion-model or IMU prediction, Tracking.cc:2800-2835 / PredictStateIMU): H2D of the images
 * and of the map points, extraction of both eyes, ComputeStereoMatches, AssignFeaturesToGrid, isInFrustum, window search and
 * the read-back are one stream of work; the host only replays the claims.  A new frame holds no map points
 * (Frame.cc:139), so frame_mp[capacity] is an OUTPUT here (-1 = none).  *rounds (may be NULL) = device rounds of the window
 * search (1 unless a candidate list was exhausted by earlier claims). */
int msorb_track_frontend(msorb_extractor* h, msorb_frame* f, const uint8_t* left, const uint8_t* right, int rows, int cols,
                         size_t stride_left, size_t stride_right, float mb, float mbf, msorb_keypoint* kps_left, uint8_t* desc_left,
                         int* n_left, msorb_keypoint* kps_right, uint8_t* desc_right, int* n_right, int capacity, float* u_right,
                         float* depth, int* n_oob, float min_x, float max_x, float min_y, float max_y, const msorb_frustum* frustum,
                         float viewing_cos_limit, int m, const float* pos_w, const float* normal, const float* max_distance,
                         const float* min_distance, const uint8_t* visit, const uint8_t* bad, const uint8_t* sparsified,
                         const uint8_t* mp_desc, const int* obs, int* frame_mp, float th, int far_points, float th_far_points,
                         float nnratio, uint8_t* track_in_view, float* proj_x, float* proj_y, float* proj_xr, float* track_depth,
                         int* scale_level, float* view_cos, int* nmatches, int* rounds);

/* ------------------------------------------------------------------------------------------------
 * TrackWithMotionModel's search (src/Tracking.cc:2833-2870): ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)
 * (src/ORBmatcher.cc:1941-2152, rectified rig / Nleft == -1) with the projection of :1962-1990 ON THE DEVICE.  The last
 * frame's points stay resident on the current frame's handle between calls (the retry at 2 * th, Tracking.cc:2861-2868, is a
 * second msorb_search_last_frame without another upload).
 * ---------------------------------------------------------------------------------------------- */
typedef struct msorb_motion_model {
    float q[4];                         /* Tcw.unit_quaternion() as Sophus stores it: x, y, z, w (:1951) */
    float t[3];                         /* Tcw.translation() */
    float fx, fy, cx, cy;               /* Pinhole mvParameters[0..3] (Pinhole.cpp:43-49) */
    float mbf;                          /* CurrentFrame.mbf (:2019) */
    int forward, backward;              /* bForward / bBackward (:1957-1958): two scalar pose operations of the caller */
} msorb_motion_model;

/* The last frame's side of the search, n entries = LastFrame.N: has_point[i] = LastFrame.mvpMapPoints[i] && !mvbOutlier[i]
 * (:1962-1965), pos_w = pMP->GetWorldPos() (3 floats), octave = LastFrame.mvKeys[i].octave (:1986), angle =
 * LastFrame.mvKeysUn[i].angle (:2044), mp_desc = pMP->GetDescriptor() (32 bytes).  Entries without a point are not read.
 * Copies the arrays (the caller's may be reused at once) and starts the upload on the frame's stream; the table then lives on
 * the handle until the next msorb_frame_set_last_points.  May be called before the frame itself is set. */
int msorb_frame_set_last_points(msorb_frame* cur, int n, const uint8_t* has_point, const float* pos_w, const int* octave,
                                const float* angle, const uint8_t* mp_desc);
/* n of the table resident on the handle (the length the proj_* arrays of msorb_search_last_frame need); -1: no table set. */
int msorb_frame_last_points_count(const msorb_frame* cur);

/* The search against the resident table: per point x3Dc = Tcw * x3Dw (Sophus' quaternion action, so3.hpp:358-367, in the
 * float convention stated in DESIGN.md), invzc < 0 / image-bounds rejections (:1973-1983), radius = th * mvScaleFactors[octave],
 * the forward / backward / default level band (:1993-1998), the window search with the occupancy and mvuRight filters
 * (:2011-2022), then — on the host, in last-frame order — the sequential claims (:2035-2038) and the rotation histogram
 * (:2040-2057, :2129-2149).  Map-point ids: last-frame point i = id i; obs[n_obs] = Observations() per id (n_obs >= n of the
 * table; ids >= n are points the current frame already holds); cur_mp[N] in / out (-1 = none).  proj_valid / proj_u / proj_v /
 * proj_ur (may be NULL, n entries): what :1962-1983 and :2019 computed — the inputs msorb_search_by_projection_frames takes, for
 * inspection.  Results equal msorb_search_by_projection_frames on those inputs. */
int msorb_search_last_frame(msorb_frame* cur, const msorb_motion_model* mm, const int* obs, int n_obs, int* cur_mp, float th,
                            int check_orientation, int* nmatches, uint8_t* proj_valid, float* proj_u, float* proj_v, float* proj_ur);

/* Frame::Frame(imLeft, imRight, ...) (Frame.cc:119-137, as msorb_extract_stereo_frame) AND the motion-model search in ONE
 * call with ONE synchronisation: the pose guess mVelocity * mLastFrame.GetPose() (Tracking.cc:2854) does not depend on the new
 * images, so images + last-frame table go up together and extraction, ComputeStereoMatches, AssignFeaturesToGrid, projection,
 * window search and the read-back are one stream of work.  A new frame holds no map points (Frame.cc:139; Tracking.cc:2857
 * clears them anyway): cur_mp[capacity] is an OUTPUT, obs has one entry per last-frame point (n of the table). */
int msorb_track_frontend_motion(msorb_extractor* h, msorb_frame* f, const uint8_t* left, const uint8_t* right, int rows, int cols,
                                size_t stride_left, size_t stride_right, float mb, float mbf, msorb_keypoint* kps_left,
                                uint8_t* desc_left, int* n_left, msorb_keypoint* kps_right, uint8_t* desc_right, int* n_right,
                                int capacity, float* u_right, float* depth, int* n_oob, float min_x, float max_x, float min_y,
                                float max_y, const msorb_motion_model* mm, const int* obs, int* cur_mp, float th,
                                int check_orientation, int* nmatches);

/* The device part of the same chain for a BATCH of frames whose features are device resident (offline throughput and the
 * measurement of the windowed Hamming rate): frame b's keypoints / descriptors / count are image b*frame_step of an
 * msorb_extract_batch output (frame_step = 2: the left images of interleaved stereo pairs), d_u_right[b*capacity ..] its
 * mvuRight (msorb_stereo_matches_batch output; NULL = none).  Per frame: frusta[b] (HOST array) and m map points in the device
 * arrays d_pos_w [n_frames][3m], d_normal, d_max_distance, d_min_distance [n_frames][m], d_flags (bit 0 visit, bit 1 isBad,
 * bit 2 mbSparsified), d_mp_desc [n_frames][m][32].  Three launches: grids, frustum + queries, window search against frames
 * that hold no map points yet.  d_topk[n_frames][m][16]: per map point the 8 best candidates in the reference's scan order —
 * 8 keypoint indices (-1 = none) then 8 distances; d_track_in_view (may be NULL) [n_frames][m]; d_cell_begin / d_cell_idx (may
 * be NULL) receive the grids ([n_frames][3073] / [n_frames][capacity]).  elapsed_ms[3] (may be NULL) = device time of the three
 * launches; *n_pairs (may be NULL; HOST) = Hamming distances evaluated by the window search. */
int msorb_track_batch(int device, int n_frames, const msorb_keypoint* d_keypoints, const uint8_t* d_descriptors,
                      const float* d_u_right, const int* d_counts, int frame_step, int capacity, float min_x, float max_x,
                      float min_y, float max_y, const float* scale_factors, int nlevels, const msorb_frustum* frusta,
                      float viewing_cos_limit, int m, const float* d_pos_w, const float* d_normal, const float* d_max_distance,
                      const float* d_min_distance, const uint8_t* d_flags, const uint8_t* d_mp_desc, float th, int far_points,
                      float th_far_points, int* d_topk, uint8_t* d_track_in_view, int* d_cell_begin, int* d_cell_idx,
                      float* elapsed_ms, unsigned long long* n_pairs);

/* MLPnPsolver's RANSAC (src/MLPnPsolver.cpp:143-266) for a pinhole camera on the device, every hypothesis at once.  Appended to ABI
 * 6002 as the Sim3 RANSAC was: MSORB_ABI_VERSION stays 6002.  The draws of :163-183 do not depend on the data, so the caller draws
 * the minimal sets of all iterations beforehand (DUtils::Random::RandomInt with the swap-with-back rule of :173-182) and hands them
 * in as sets of six indices; computePose (:399-701) and CheckInliers (:305-336) then run for all of them in one launch, and a
 * second launch applies the loop's sequential rule (:212-263) to the counts in hypothesis order: starting from best_inliers_in
 * (mnBestInliers), a hypothesis with count >= min_inliers (mRansacMinInliers) raises the best when count > best, and the scan
 * stops at the first hypothesis with count > min_inliers, which is handed out whether or not it is the best (Refine(), :338-396,
 * computes into a local nothing reads and counts the current hypothesis again).
 *   problem   n correspondences, n_hyp sets, cam = fx, fy, cx, cy of mpCamera (Pinhole only)
 *   result    winner: converged, the hypothesis the loop returned at; otherwise the last one that raised the best (-1: none did;
 *             the record is then all zero); converged: Refine() returned true there; consumed: the iterations the loop went
 *             through (mnIterations advances by it: winner + 1 when converged, n_hyp otherwise); n_inliers = mnInliersi of the
 *             winner, R (row major) / t = its mRi / mti, Tcw = mRefinedTcw / mBestTcw (row major): R and t narrowed to float
 * Problem i owns the correspondences [corr_offset[i], corr_offset[i+1]) of p2d (2 floats each: mvP2D, from which the bearings are
 * taken as Pinhole::unproject followed by / z, :78-80), p3d_w (3 floats each: mvP3Dw) and max_err (mvMaxError) and the hypotheses
 * [hyp_offset[i], hyp_offset[i+1]) of sets (6 indices into the problem's own correspondences); both offset arrays start at 0 and
 * advance by n / n_hyp.  inlier_out [per correspondence] = the winner's mvbInliersi (0 without a winner); counts_out [per
 * hypothesis] (may be NULL) = every hypothesis' mnInliersi, also of those behind a converged winner; hyp_pose_out (may be NULL)
 * [per hypothesis] = R (9, row major) then t (3); hyp_flags_out (may be NULL) [per hypothesis]: bit 0 the planar branch was taken,
 * bits 1-3 the Gauss-Newton updates applied (0-5), bit 4 the loop was left by the break of :787.  computePose is double, one
 * rounded operation per reference operator (csrc/mlpnp_device.h), with the choices the reference leaves to Eigen fixed there, so
 * bit parity with a compiled Eigen / libm is not pinned; CheckInliers narrows to float where the reference
 * does.  The N-point computePose of Refine() is dead work and is not done.  Non-finite poses are results: they count no inlier
 * and take part in the rule.
 * MSORB_E_INVALID, before anything is launched and with every output untouched: n < 6, n_hyp < 1, offsets that do not match, an
 * index of a set that is negative, >= n or repeated within its set, a null required array.  n_problems == 0 is MSORB_OK.  Flat host
 * arrays, one upload, two launches, one read-back.  Two calls on the same input return the same bits, and a batch returns the
 * bits of the single calls.  Re-entrant: every calling thread has its own stream and staging.  *elapsed_ms (may be NULL) = device
 * time of the two launches. */
typedef struct msorb_mlpnp_problem {
    int n, n_hyp, min_inliers, best_inliers_in;
    float cam[4];
} msorb_mlpnp_problem;
typedef struct msorb_mlpnp_result {
    int winner, converged, consumed, n_inliers;
    float Tcw[16];
    double R[9], t[3];
} msorb_mlpnp_result;
int msorb_mlpnp_ransac_batch(int device, int n_problems, const msorb_mlpnp_problem* problems, const int* corr_offset,
                             const int* hyp_offset, const float* p2d, const float* p3d_w, const float* max_err, const int* sets,
                             uint8_t* inlier_out, int* counts_out, double* hyp_pose_out, uint8_t* hyp_flags_out,
                             msorb_mlpnp_result* results, float* elapsed_ms);

/* TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc:41-129) for a pinhole camera on the device: the monocular
 * initialisation between msorb_search_for_initialization and CreateInitialMapMonocular.  Appended to ABI 6002 as the MLPnP RANSAC
 * was: MSORB_ABI_VERSION stays 6002.  One problem per call: no caller has more.  The reference draws all minimal sets before its loops
 * (:79-98) and has no early exit, so the caller draws them (DUtils::Random::SeedRandOnce(0), RandomInt, the swap-with-back rule of
 * :83-98) and hands them in; all n_hyp homographies and all n_hyp fundamental matrices are then computed and scored over every match
 * in one launch, a second launch folds the scores (:172-177, :223-228), takes Reconstruct's branch and forms the 8 (ReconstructH,
 * :582-690) or 4 (ReconstructF / DecomposeE) motion hypotheses, a third runs CheckRT (:786-901) for each of them; the host part of
 * the entry takes acos with the host's libm and applies the closing rule (:505-568, :693-733).
 *   keys1 [n1 x 2], keys2 [n2 x 2]   the pt of mvKeysUn of the reference / current frame; Normalize (:737-784) runs over ALL of them
 *   matches12 [n1]                   index into keys2 or -1; the match list is its entries >= 0 in ascending order of i (:55-64)
 *   sets [n_hyp x 8]                 indices into the match list (mvSets)
 *   fx, fy, cx, cy, sigma            K as Pinhole::toK_ gives it (no skew), mSigma
 *   h_ratio                          the constant of :119: the reference has 0.50 (its comment names the older 0.40-0.45)
 *   min_parallax, min_triangulated   the reference passes 1.0 and 50
 * result: ok = Reconstruct's return value; branch 0 no model (SH + SF == 0), 1 homography, 2 fundamental; winner_h / winner_f the
 * hypotheses the two folds kept (-1: no score exceeded 0); model = the branch's H21 / F21 (row major); n_motion 8, 4 or 0 (the
 * return of :597-600); motion_R / motion_t every motion hypothesis in the reference's order; n_good / cosine / parallax per motion
 * hypothesis: CheckRT's return value, the accepted cosParallax at sorted index min(50, nGood - 1), and acos of it in degrees;
 * chosen = the hypothesis handed out (-1: none), R / t = T21 (zero when !ok); n_inliers = the N of :478-481 / :574-577.
 * triangulated [n1] / p3d [n1 x 3] = vbTriangulated and the chosen hypothesis' vP3D, indexed by the keypoint of frame 1 (all zero
 * when !ok; ReconstructH hands vbTriangulated out and leaves vP3D unassigned, :725-731: p3d here holds the points it dropped).
 * inlier_out [per match] = the branch winner's vbMatchesInliers.  hyp_score_out / hyp_count_out [2 n_hyp] and hyp_mask_out
 * [2 n_hyp x matches] (each may be NULL): every hypothesis' score, inlier count and mask, the homographies first.
 * Float, one rounded operation per reference operator (csrc/two_view_device.h), with what the reference leaves to Eigen fixed there
 * (DESIGN.md section 15), so bit parity with a compiled Eigen is not pinned.  A match whose triangulation has x3Dh(3) == 0 counts
 * as not finite (the reference reads an unassigned vector there).
 * MSORB_E_INVALID, before anything is launched and with every output untouched: fewer than 8 matches, n_hyp < 1, a set index that
 * is negative, beyond the match count or repeated within its set, a match index >= n2, a null required array (the three hyp_*
 * outputs and elapsed_ms are optional).  More than 32768 matches: MSORB_E_CAPACITY.  One upload, three launches, one read-back; two
 * calls on the same input return the same bits.  Re-entrant: every calling thread has its own stream and staging.  *elapsed_ms
 * (may be NULL) = device time of the three launches. */
typedef struct msorb_two_view_result {
    int ok, branch, winner_h, winner_f, n_motion, chosen, n_inliers;
    float SH, SF, RH;
    float R[9], t[3];
    float model[9];
    int n_good[8];
    float parallax[8], cosine[8];
    float motion_R[72], motion_t[24];
} msorb_two_view_result;
int msorb_two_view_reconstruct(int device, int n1, const float* keys1, int n2, const float* keys2, const int* matches12,
                               int n_hyp, const int* sets, float fx, float fy, float cx, float cy, float sigma, double h_ratio,
                               float min_parallax, int min_triangulated, msorb_two_view_result* result, uint8_t* triangulated,
                               float* p3d, uint8_t* inlier_out, float* hyp_score_out, int* hyp_count_out, uint8_t* hyp_mask_out,
                               float* elapsed_ms);

/* Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1410-1675 for loop closing, :1677-1985 for map merging; not the 4-DoF
 * inertial form) after the gathering loops, on the device: g2o's 7-DoF pose graph of VertexSim3Expmap and EdgeSim3 with the
 * identity for information and no kernel, the edge's NUMERIC Jacobian (central differences of 1e-9 through oplus), Levenberg from
 * the user lambda 1e-16, in double.  Appended to ABI 6002 as the bundle adjustments were: MSORB_ABI_VERSION stays 6002.
 * vertices [n_vertices]: the estimate (q = x, y, z, w; nothing normalises it), fixed (setFixed) and fix_scale (_fix_scale: the
 * update's seventh entry is zeroed).  Edge e joins vertices edge_v0[e] -> edge_v1[e] with measurement Sjw * Swi as 8 doubles
 * (q[4], t[3], s); error = log(C * v0 * v1^-1).  Several edges on one pair are legal.  g2o's active set holds: an edge with two
 * fixed ends enters neither the cost nor H; a free vertex without an active edge keeps its estimate bit for bit.  The 7 Kf x 7 Kf
 * system (Kf: free vertices with an active edge, in the caller's order) is solved DENSELY by the blocked L D L^T of
 * msorb_ldlt_solve, unpivoted, where the reference runs a sparse Cholesky.  estimates_out [8 per vertex]: q, t, s.
 * Errors: MSORB_E_ARG for an edge that names a vertex out of range or has v0 == v1, a null required array, a negative count.
 * More than msorb_essential_graph_capacity() free vertices in the system, or no room on the device for it: MSORB_E_CAPACITY,
 * nothing launched, no output written.  No active edge: zero iterations and the estimates as they came.  Two calls on the same
 * input return the same bits.  Re-entrant like msorb_local_ba.  *elapsed_ms (may be NULL): device time. */
typedef struct msorb_eg_vertex {
    double q[4], t[3], s;
    int32_t fixed, fix_scale;
} msorb_eg_vertex;
typedef struct msorb_eg_result {
    int32_t status;            /* 0 */
    int32_t iterations, trials, rejected_trials;
    int32_t solver_failures;   /* trials whose factorisation met a pivot that was not positive */
    int32_t stop;              /* 0: every iteration ran; 1: Terminate (ten trials, or rho == 0); 2: the fork's _nBad >= 3 */
    double chi2_initial, chi2_final, lambda_final;
} msorb_eg_result;
int msorb_essential_graph_capacity(void);              /* free vertices: 1024 (the system is 7168^2 doubles = 411 MB) */
int msorb_essential_graph(int device, int n_vertices, const msorb_eg_vertex* vertices, int n_edges, const int* edge_v0,
                          const int* edge_v1, const double* measurements, int iterations, double* estimates_out,
                          msorb_eg_result* result, float* elapsed_ms);
/* Device ms of the calling thread's last msorb_essential_graph call: linearise, assemble, solve, trial.  Needs
 * MSORB_LOCAL_BA_STAGES=1 in the environment before the library is loaded (MSORB_E_ARG otherwise, zeros). */
int msorb_essential_graph_stage_ms(float ms[4]);

/* Optimizer::OptimizeEssentialGraph4DoF (src/Optimizer.cc:5174-5458: what LoopClosing::CorrectLoop runs on an inertial map) after
 * the gathering loops, on the device: g2o's pose graph of VertexPose4DoF (yaw about the world's z and a world-frame translation,
 * through ImuCamPose::UpdateW) and Edge4DoF (LogSO3 of the rotation residual, the translation residual) with the information
 * diag(1e3, 1e3, 1, 1, 1, 1), no kernel, the edge's NUMERIC Jacobian (central differences of 1e-9 through oplus) and Levenberg
 * from computeLambdaInit = 1e-5 max |H(j,j)|, in double.  Appended to ABI 6002: MSORB_ABI_VERSION stays 6002.
 * vertices [n_vertices], 3x3 matrices row major: the camera pose Rcw, tcw and the body pose Rwb, twb the estimate starts from
 * (inputs of their own: ImuCamPose(pKF) does not derive one from the other), the constants Rcb, tcb, and fixed (setFixed).
 * Edge e joins vertices edge_v0[e] -> edge_v1[e] with measurement dRij[9], dtij[3] (12 doubles).  Several edges on one pair are
 * legal.  g2o's active set holds: an edge with two fixed ends enters neither the cost nor H; a free vertex without an active edge
 * keeps its pose bit for bit.  The 4 Kf x 4 Kf system (Kf: free vertices with an active edge, in the caller's order) is solved
 * DENSELY by the blocked L D L^T of msorb_ldlt_solve, unpivoted, where the reference runs a sparse Cholesky.
 * poses_out [12 per vertex]: Rcw[9], tcw[3].
 * Errors: MSORB_E_ARG for an edge that names a vertex out of range or has v0 == v1, a null required array, a negative count.
 * More than msorb_essential_graph4_capacity() free vertices in the system, or no room on the device for it: MSORB_E_CAPACITY,
 * nothing launched, no output written.  No active edge: zero iterations and the poses as they came.  Two calls on the same
 * input return the same bits.  Re-entrant like msorb_local_ba.  *elapsed_ms (may be NULL): device time. */
typedef struct msorb_eg4_vertex {
    double Rcw[9], tcw[3], Rwb[9], twb[3], Rcb[9], tcb[3];
    int32_t fixed, reserved;
} msorb_eg4_vertex;
typedef struct msorb_eg4_result {
    int32_t status;            /* 0 */
    int32_t iterations, trials, rejected_trials;
    int32_t solver_failures;   /* trials whose factorisation met a pivot that was not positive */
    int32_t stop;              /* 0: every iteration ran; 1: Terminate (ten trials, or rho == 0); 2: the fork's _nBad >= 3 */
    double chi2_initial, chi2_final, lambda_final;
    double lambda_initial;     /* computeLambdaInit at the first linearisation */
} msorb_eg4_result;
int msorb_essential_graph4_capacity(void);             /* free vertices: 1792 (the system is 7168^2 doubles = 411 MB) */
int msorb_essential_graph4(int device, int n_vertices, const msorb_eg4_vertex* vertices, int n_edges, const int* edge_v0,
                           const int* edge_v1, const double* measurements, int iterations, double* poses_out,
                           msorb_eg4_result* result, float* elapsed_ms);
/* Device ms of the calling thread's last msorb_essential_graph4 call: linearise, assemble, solve, trial.  Needs
 * MSORB_LOCAL_BA_STAGES=1 in the environment before the library is loaded (MSORB_E_ARG otherwise, zeros). */
int msorb_essential_graph4_stage_ms(float ms[4]);

/* Optimizer::InertialOptimization (src/Optimizer.cc:3050-3227, :3230-3384, :3386-3491: IMU initialisation, the bias refit after a
 * merge, ScaleRefinement) after the gathering loops, on the device, the whole optimize(its) in ONE launch: EdgeInertialGS
 * (src/G2oTypes.cc:596-718) between consecutive KeyFrames with every pose fixed, EdgePriorAcc / EdgePriorGyro on the biases, the
 * vertices VertexVelocity, VertexGyroBias, VertexAccBias, VertexGDir, VertexScale, Levenberg or Gauss-Newton, in double with the
 * preintegration's bias correction in float as the reference has it.  The three overloads are one graph with different vertices
 * fixed: the free_* flags.  Appended to ABI 6002: MSORB_ABI_VERSION stays 6002.
 * kfs [n_kf]: the body pose Rwb (row major), twb and the velocity the estimate starts from; has_velocity_vertex = 0 for a KeyFrame
 * the reference gives no vertex (mnId > maxKFid): no edge may name it.  edges [n_edges] in the order of the reference's edge list:
 * the members of IMU::Preintegrated as floats (3x3 row major; bias = b: ba then bg), and info = the FULL 9x9 information the
 * edge's constructor leaves (:604-612), row major, all 81 entries used.  Every KeyFrame may have one incoming and one outgoing
 * edge and the edges may form no cycle (chains): anything else is MSORB_E_CAPACITY ("not handled"), as is n_kf above
 * msorb_inertial_optimization_capacity().  A KeyFrame without an edge has no active vertex: v_out returns its velocity as it came.
 * with_priors: the two prior edges exist (first and second overload), information prior_a I and prior_g I.  They are active
 * only while the biases are free (g2o's initializeOptimization drops an edge whose vertices are all fixed): with free_biases == 0
 * they enter neither chi2 nor n_active_edges.  n_edges == 0 is valid: gravity direction, scale and velocities are then
 * inactive, and without a free bias under a prior nothing is optimised (status 1, g2o's "0 vertices to optimize").
 * H is block-tridiagonal (3x3, velocities in chain order) with a dense border of at most 9 (bg, ba, gravity direction, scale):
 * solved by block cyclic reduction and a Schur complement on the border, unpivoted L D L^T throughout, where the reference runs a
 * sparse Cholesky.  v_out [3 n_kf]; edge_chi2 [n_edges] or NULL: chi2() of every inertial edge at the returned estimate.
 * Errors, before anything is launched and with no output written: MSORB_E_INVALID for a null required pointer, a negative count,
 * an index out of range, kf_prev == kf_cur, an edge on a KeyFrame without velocity vertex, iterations < 0 or > 10000, an unknown algorithm,
 * a non-finite input.  Two calls on the same input return the same bits.  Re-entrant.  *elapsed_ms (may be NULL): device time. */
typedef struct msorb_inertial_keyframe { double Rwb[9], twb[3], v[3]; int32_t has_velocity_vertex, reserved; } msorb_inertial_keyframe;
typedef struct msorb_inertial_edge {
    int32_t kf_prev, kf_cur;
    float dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], bias[6], dT;
    double info[81];
} msorb_inertial_edge;
typedef struct msorb_inertial_problem {
    double Rwg[9], scale, bg[3], ba[3], prior_g, prior_a;
    int32_t free_velocities, free_biases, free_gdir, free_scale, with_priors;
    int32_t algorithm;          /* 0 Levenberg, 1 Gauss-Newton */
    int32_t user_lambda_init;   /* 1: setUserLambdaInit(1e3); 0: computeLambdaInit = 1e-5 max |H(j,j)| */
    int32_t huber;              /* 1: RobustKernelHuber with delta 1 on every inertial edge */
    int32_t iterations, reserved;
} msorb_inertial_problem;
typedef struct msorb_inertial_result {
    double Rwg[9], scale, bg[3], ba[3], chi2_initial, chi2_final;
    int32_t status;             /* 0 optimised; 1 no vertex to optimise (optimize returns -1, nothing moved); 2 Gauss-Newton's
                                   solve failed: update(x) ran with the x it held, then the loop stopped (optimize returns 0) */
    int32_t iterations, rejected_trials, n_active_edges;
} msorb_inertial_result;
int msorb_inertial_optimization_capacity(void);        /* KeyFrames: 4096 */
int msorb_inertial_optimization(int device, const msorb_inertial_problem* p, int n_kf, const msorb_inertial_keyframe* kfs,
                                int n_edges, const msorb_inertial_edge* edges, double* v_out, double* edge_chi2,
                                msorb_inertial_result* r, float* elapsed_ms);

/* Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:4422-4779) and PoseInertialOptimizationLastFrame (:4781-5172)
 * after their gathering loops, for pinhole mono / stereo frames without a second camera: the four rounds of Gauss-Newton, the
 * classifications, the recovery arm and the final Hessian in ONE launch, in double with the preintegration's bias correction in
 * float as the reference has it; the marginalisation (:2975-3048) and ConstraintPoseImu's constructor (G2oTypes.h:711-722) run on
 * the host inside the call.  Appended to ABI 6002: MSORB_ABI_VERSION stays 6002.
 * form 0: the other end is the last KeyFrame, its four vertices fixed (15 unknowns).  form 1: the other end is the previous frame,
 * free, under EdgePriorPoseImu with the information H and the linearisation point `prior` (30 unknowns, the frame's first).
 * frame / other: {Rwb (row major), twb, v, bg, ba} the estimates start from.  Rcw, tcw: GetPose() widened (ImuCamPose does not
 * derive them from Rwb / twb); Rcb, tcb: mTcb; tbc: mTbc.translation().  pre: the preintegration of the inertial edge (kf_prev /
 * kf_cur ignored; info = the full 9x9 information of EdgeInertial's constructor).  info_gyro, info_acc: the 3x3 informations of
 * EdgeGyroRW / EdgeAccRW, row major.  rec_init: bRecInit.  n: observations (u_right >= 0 = stereo; close = mTrackDepth < 10.f).
 * Result: est = the frame's four vertices in double; Rwb_f, twb_f, v_f = what SetImuPoseVelocity receives; n_initial - n_bad is
 * the reference's return value; iterations[k] = passes of round k (-1: round not run), solve_failed[k] = its solve failed (the
 * update ran with the x the solver held; x starts at zero); H_raw = the 15x15 (form 0) or 30x30 (form 1, previous frame first)
 * Hessian of :4743-4773 / :5120-5162, row major; H_prior = the H the new ConstraintPoseImu holds.
 * Errors, before anything is launched and with no output written: MSORB_E_INVALID for a null required pointer, a negative count,
 * an unknown form, offsets that do not match the problems' n, a non-finite input.  Two calls on the same input return the same
 * bits.  Re-entrant. */
typedef struct msorb_pose_inertial_state { double Rwb[9], twb[3], v[3], bg[3], ba[3]; } msorb_pose_inertial_state;
typedef struct msorb_pose_inertial_problem {
    int32_t form, rec_init, n, reserved;
    msorb_pose_inertial_state frame, other, prior;
    double Rcw[9], tcw[3], Rcb[9], tcb[3], tbc[3];
    float fx, fy, cx, cy, mbf, reserved_f;
    msorb_inertial_edge pre;
    double info_gyro[9], info_acc[9];
    double H[225];              /* form 1: mpcpi->H, row major */
} msorb_pose_inertial_problem;
typedef struct msorb_pose_inertial_result {
    msorb_pose_inertial_state est;
    float Rwb_f[9], twb_f[3], v_f[3];
    int32_t n_initial, n_bad, n_inliers;
    int32_t iterations[4], solve_failed[4];
    double H_raw[900];
    double H_prior[225];
} msorb_pose_inertial_result;
int msorb_pose_inertial_optimization_capacity(void);   /* observations a problem keeps in registers: 2048 */
int msorb_pose_inertial_optimization_batch(int device, int n_problems, const msorb_pose_inertial_problem* problems,
                                           const int* obs_offset, const float* xy, const float* u_right, const float* inv_sigma2,
                                           const float* pos_w, const uint8_t* close, uint8_t* outlier_out,
                                           msorb_pose_inertial_result* results, float* elapsed_ms);
/* The frame form over the keypoint table resident on the handle (rectified input, as msorb_frame_pose_optimization): has_point
 * [N], pos_w [N, 3], close [N]; outlier [N] is written where has_point is set.  Bit-equal to the flat form. */
int msorb_frame_pose_inertial_optimization(msorb_frame* f, const msorb_pose_inertial_problem* p, const uint8_t* has_point,
                                           const float* pos_w, const uint8_t* close, const float* inv_level_sigma2, int nlevels,
                                           uint8_t* outlier, msorb_pose_inertial_result* r);

/* Optimizer::LocalInertialBA (src/Optimizer.cc:2431-2973) after its gathering loops, on the device, for pinhole KeyFrames without a
 * second camera (the mpCamera2 arm of :2820-2853 is not restated; FullInertialBA is msorb_full_inertial_ba below, MergeInertialBA msorb_merge_inertial_ba): EdgeMono /
 * EdgeStereo over ImuCamPose and the points, EdgeInertial, EdgeGyroRW and EdgeAccRW along the chain of KeyFrames, g2o's Levenberg
 * with setUserLambdaInit, the points eliminated by the Schur complement, in double with the preintegration's bias correction in
 * float as the reference has it.  The whole optimize() is ONE launch of one workgroup.  Appended to ABI 6002: MSORB_ABI_VERSION
 * stays 6002.
 * problem: large = bLarge: lambda 1e-2 and 4 iterations against 1e0 and 10 (:2435-2440, :2547-2555), and no FAIL rule;
 * iterations > 0 replaces the 4 / 10.
 * kfs [n_kf]: everything VertexPose(pKF) / ImuCamPose(pKF) reads, in the conventions of msorb_pose_inertial_problem: Rcw / tcw =
 * GetPose() widened, not derived.  kind: 0 = free, with pose, velocity and both biases (15 unknowns); 1 = fixed, with inertial
 * vertices (the KeyFrame before the window, or the window's oldest without mPrevKF); 2 = fixed pose only; 3 = free pose only (6
 * unknowns), which msorb_merge_inertial_ba alone accepts: here and in msorb_full_inertial_ba a kind above 2 is MSORB_E_INVALID,
 * and the caller does not hand such a window over.
 * iedges [n_inertial]: pre.kf_prev / pre.kf_cur index kfs; pre.info = the full 9x9 of EdgeInertial's constructor; info_gyro /
 * info_acc (:2673, :2680) row major; huber: RobustKernelHuber of delta sqrt(16.92) (:2657-2667); downweight: information() *
 * 1e-2, applied in double inside the library (:2665).  One incoming and one outgoing edge per KeyFrame, no cycle: anything else
 * is MSORB_E_CAPACITY, as are more free KeyFrames than msorb_local_inertial_ba_capacity().  An edge between two fixed KeyFrames
 * is not active.
 * Visual edges: msorb_local_ba's arrays in point-major order; u_right >= 0 = EdgeStereo, else EdgeMono (cam_idx 0); inv_sigma2 =
 * mvInvLevelSigma2[octave] / unc2 as the float the host divides (:2771-2773); point_close [n_points] = mTrackDepth < 10.f.
 * Result: status 0 = optimised; 1 = the FAIL rule of :2911 held; 2 = no free KeyFrame and no edge.  chi2_initial / chi2_final =
 * the two activeRobustChi2 of :2865 / :2867, err / err_end their float narrowings.  chi2_final and every edge's chi2 of the
 * classification (:2876-2904, which reads chi2() without computeError()) belong to the state the LAST TRIAL wrote, accepted or
 * not; isDepthPositive() reads the returned estimate.  With status 1 or 2 every estimate output repeats its input and no flag is
 * set.  kf_out [n_kf]: the doubles, and what the setters receive: Rcw / tcw narrowed (SetPose, :2937), v (:2943) and the bias in
 * IMU::Bias's order, acc then gyro (:2946-2948); a fixed KeyFrame's repeat its input.  pos_out [3 n_points], pos_d (may be NULL),
 * edge_outlier [n_edges] = vToErase.  No stop flag: the reference installs it after optimize() (:2868-2869).
 * Errors, before anything is launched and with no output written: MSORB_E_INVALID for a null required pointer, a negative count,
 * an index out of range, kf_prev == kf_cur, edges that are not point-major, an inertial edge on a kind 2 KeyFrame, a non-finite
 * input, an unknown kind.  Two calls on the same input return the same bits.  Re-entrant.  *elapsed_ms (may be NULL): device time. */
typedef struct msorb_iba_problem { int32_t large, iterations, reserved[2]; } msorb_iba_problem;
typedef struct msorb_iba_keyframe {
    double Rwb[9], twb[3], v[3], bg[3], ba[3], Rcw[9], tcw[3], Rcb[9], tcb[3], tbc[3];
    float fx, fy, cx, cy, mbf;
    int32_t kind;
} msorb_iba_keyframe;
typedef struct msorb_iba_inertial_edge {
    msorb_inertial_edge pre;
    double info_gyro[9], info_acc[9];
    int32_t huber, downweight;
} msorb_iba_inertial_edge;
typedef struct msorb_iba_keyframe_out {
    double Rwb[9], twb[3], Rcw[9], tcw[3], v[3], bg[3], ba[3];
    float Rcw_f[9], tcw_f[3], v_f[3], bias_f[6], reserved_f;
} msorb_iba_keyframe_out;
typedef struct msorb_iba_result {
    int32_t status, iterations, trials, rejected_trials, n_outliers, reserved;
    double chi2_initial, chi2_final, lambda_final;
    float err, err_end;
} msorb_iba_result;
int msorb_local_inertial_ba_capacity(void);            /* free KeyFrames: 25 */
int msorb_local_inertial_ba(int device, const msorb_iba_problem* p, int n_kf, const msorb_iba_keyframe* kfs, int n_inertial,
                            const msorb_iba_inertial_edge* iedges, int n_points, const float* pos_w, const uint8_t* point_close,
                            int n_edges, const int* edge_kf, const int* edge_point, const float* xy, const float* u_right,
                            const float* inv_sigma2, msorb_iba_keyframe_out* kf_out, float* pos_out, double* pos_d,
                            uint8_t* edge_outlier, msorb_iba_result* r, float* elapsed_ms);

/* Optimizer::FullInertialBA (src/Optimizer.cc:366-756) after its gathering loops, on the device, for pinhole KeyFrames without a
 * second camera (the mpCamera2 arm of :643-673 is not restated): g2o's optimize(its) over the whole inertial map, as
 * LocalMapping::InitializeIMU (init = 1, then init = 0) and the global BA after a loop closure on an inertial map run it.  The host
 * drives g2o's Levenberg loop launch by launch over the whole chip and looks at *stop_flag (may be NULL) where g2o calls
 * terminate(); the reduced system is factored by the blocked L D L^T of msorb_bundle_adjustment.  In double, with the
 * preintegration's bias correction in float as the reference has it.  Appended to ABI 6002: MSORB_ABI_VERSION stays 6002.
 * problem: init = bInit.  init = 0: per free KeyFrame pose, velocity, gyro bias, acc bias; EdgeInertial, EdgeGyroRW, EdgeAccRW.
 * init = 1: per free KeyFrame pose and velocity, ONE gyro and one acc bias shared by every EdgeInertial, starting at bg0 / ba0
 * (the bias of the last KeyFrame the loop of :393-425 visits), no random-walk edge (info_gyro / info_acc are ignored),
 * EdgePriorGyro / EdgePriorAcc with prior_g / prior_a times the identity and bprior = 0.  iterations = its; lambda starts at 1e-5
 * (setUserLambdaInit); no classification, no FAIL rule.
 * kfs, iedges and the visual edges: msorb_local_inertial_ba's records.  huber / downweight are honoured as given (the reference:
 * huber on every edge, no downweight).  With init = 0 an inertial edge between two fixed KeyFrames is not active; with init = 1 it
 * is, because the shared biases are free.  No fixed KeyFrame at all is the normal case.  A point none of whose edges ends at a
 * free KeyFrame is no vertex and its edges do not count (:677-680): point_included [n_points] = 0 and its position repeats.
 * Result: status 0 = optimised; 2 = nothing to optimise (no KeyFrame, or init = 0 without a free one); 3 = *stop_flag was set
 * before optimize() (:683-685); with 2 and 3 every output repeats its input.  n_outliers, err, err_end = 0.  reserved = the number of
 * trials whose factorisation met a pivot that was not positive (g2o's rule then takes the cost as DBL_MAX and may still accept the
 * trial).  The solve is dense and unpivoted: without a fixed KeyFrame the four gauge directions are held by lambda alone, and on maps of
 * about 25 KeyFrames and more rounding decides whether a pivot is positive.  A call with reserved != 0 is outside what is claimed:
 * msorb_host::FullInertialBA hands such a map back to g2o.  kf_out as
 * msorb_local_inertial_ba's; a fixed KeyFrame's repeats its input, except that with init = 1 every KeyFrame with inertial vertices
 * (kind 0 and 1) receives the shared biases (:720-733).
 * Errors as msorb_local_inertial_ba's, nothing written before the last of them has passed; inertial edges that are not chains, or
 * more free KeyFrames than msorb_full_inertial_ba_capacity(init) (477 / 795: a dense square of 7168 unknowns), are
 * MSORB_E_CAPACITY.  *r, *elapsed_ms and the output arrays are first written when the call has succeeded: a call that returns an
 * error, MSORB_E_HIP included, leaves them as they were (msorb_merge_inertial_ba does the same).
 * Two calls on the same input return the same bits.  Re-entrant.  *elapsed_ms (may be NULL): device time.
 * msorb_full_inertial_ba_stage_ms: with MSORB_FULL_INERTIAL_BA_STAGES=1 in the environment, the calling thread's last call's device
 * time per stage: linearise, assemble, Schur, solve, trial. */
typedef struct msorb_fiba_problem {
    int32_t init, iterations;
    float prior_g, prior_a;
    double bg0[3], ba0[3];
} msorb_fiba_problem;
int msorb_full_inertial_ba_capacity(int init);
int msorb_full_inertial_ba_stage_ms(float ms[5]);
int msorb_full_inertial_ba(int device, const msorb_fiba_problem* p, int n_kf, const msorb_iba_keyframe* kfs, int n_inertial,
                           const msorb_iba_inertial_edge* iedges, int n_points, const float* pos_w, int n_edges, const int* edge_kf,
                           const int* edge_point, const float* xy, const float* u_right, const float* inv_sigma2,
                           const volatile int* stop_flag, msorb_iba_keyframe_out* kf_out, float* pos_out, double* pos_d,
                           uint8_t* point_included, msorb_iba_result* r, float* elapsed_ms);

/* Optimizer::MergeInertialBA (src/Optimizer.cc:3918-4420) after its gathering loops, on the device, for pinhole KeyFrames without a
 * second camera: the welding bundle adjustment that LoopClosing runs when two inertial maps are merged.  The engine is
 * msorb_full_inertial_ba's (init = 0): the host drives g2o's Levenberg loop launch by launch and looks at *stop_flag (may be NULL)
 * where g2o calls terminate(); the blocked L D L^T solves the reduced system.  Appended to ABI 6002: MSORB_ABI_VERSION stays 6002.
 * kfs: msorb_local_inertial_ba's records with one more kind.  kind 0: both temporal windows and the covisible KeyFrame an inertial
 * edge reaches (15 unknowns); kind 3: a covisible KeyFrame whose pose is free and whose velocity and bias vertices no edge reaches
 * (g2o's active set leaves them out): 6 unknowns, its v / bg / ba outputs repeat the input; kind 1 / 2: fixed.  Unknowns: 6 per free
 * KeyFrame, then 9 per free KeyFrame of kind 0.  A free KeyFrame that no edge reaches is no vertex: it has no row and its output
 * repeats its input.  (A kind 0 KeyFrame that only visual edges reach keeps its nine rows, which nothing moves; g2o would number it
 * as a kind 3, and msorb_host::MergeInertialBA hands it over as one.)  A point none of whose edges ends at a free KeyFrame is no vertex either: point_included = 0, its position
 * repeats and its edges are not flagged.
 * iedges: huber / downweight are honoured as given (the reference: huber on every edge, no downweight, :4158-4185).  An inertial
 * edge on a kind 2 or kind 3 KeyFrame is MSORB_E_INVALID.  Several disjoint chains are normal; forks and cycles are
 * MSORB_E_CAPACITY, as are more unknowns than msorb_merge_inertial_ba_capacity() (7168, the side of the blocked solve's square).
 * Visual edges: point-major; u_right >= 0 = EdgeStereo; inv_sigma2 = mvInvLevelSigma2[octave] (:4272, :4293: no division by unc2).
 * problem: iterations > 0 replaces the 8 of :4317; large is ignored.  lambda starts at 1e3 (:4047).  No second round, no FAIL rule.
 * edge_outlier [n_edges] = vToErase: chi2() > 5.991f (mono) / 7.815f (stereo) and NO depth test (:4322-4349).  chi2() is read
 * without computeError(): it belongs to the state the last trial wrote, accepted or not, as in msorb_local_inertial_ba.
 * Result: status 0 = optimised; 2 = nothing to optimise (no free KeyFrame that an edge reaches); 3 = *stop_flag was set before
 * optimize() (:4312-4314), or it rose before the first iteration began: g2o would then complete zero iterations and the reference
 * would classify errors that were never computed, so that call too is handed back untouched.  With 2 and 3 every output repeats its
 * input and no flag is set.  n_outliers = flags set; reserved = trials whose factorisation met a pivot that was not positive, as
 * msorb_full_inertial_ba counts them; err, err_end = 0.
 * Errors as msorb_local_inertial_ba's, before any launch and with no output written.  Two calls on the same input return the same
 * bits.  Re-entrant per calling thread.  *elapsed_ms (may be NULL): device time.  msorb_merge_inertial_ba_stage_ms: with
 * MSORB_MERGE_INERTIAL_BA_STAGES=1 in the environment, the calling thread's last call's device time per stage, as
 * msorb_full_inertial_ba_stage_ms. */
int msorb_merge_inertial_ba_capacity(void);            /* unknowns: 7168 */
int msorb_merge_inertial_ba_stage_ms(float ms[5]);
int msorb_merge_inertial_ba(int device, const msorb_iba_problem* p, int n_kf, const msorb_iba_keyframe* kfs, int n_inertial,
                            const msorb_iba_inertial_edge* iedges, int n_points, const float* pos_w, int n_edges, const int* edge_kf,
                            const int* edge_point, const float* xy, const float* u_right, const float* inv_sigma2,
                            const volatile int* stop_flag, msorb_iba_keyframe_out* kf_out, float* pos_out, double* pos_d,
                            uint8_t* edge_outlier, uint8_t* point_included, msorb_iba_result* r, float* elapsed_ms);

/* The second Optimizer::LocalBundleAdjustment (pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag; src/Optimizer.cc:3494-3915) after its
 * gathering loops, on the device, for pinhole KeyFrames: the welding bundle adjustment that LoopClosing::MergeLocal runs when the
 * merged maps are not both inertial (LoopClosing.cc:1571).  The engine, the arrays and the point-major edge order are
 * msorb_local_ba's, the blocked solve and the capacity and memory check msorb_bundle_adjustment's.  Appended to ABI 6002:
 * MSORB_ABI_VERSION stays 6002.  What the routine does that no other does, it optimises twice over two graphs:
 *   round 1  optimize(5), Huber kernels of width (float)sqrt(5.99) (mono) / (float)sqrt(7.815) (stereo) on every edge (:3607-3608);
 *   levels   chi2() > 5.991 / 7.815, compared in double, or !isDepthPositive() puts an edge on level 1; every kernel is switched
 *            off (:3726-3753).  No computeError() precedes it: chi2() belongs to the state of round 1's last trial, accepted or
 *            not; the depth is the estimate's;
 *   round 2  initializeOptimization(0), optimize(10): the level-0 edges only.  A free KeyFrame or a point that no level-0 edge
 *            reaches is not in that problem: it keeps, bit for bit, what round 1 left.  lambda, ni and the count of bad
 *            iterations start anew;
 *   flags    the same test (:3769-3803): an edge of round 2 with the chi2 of round 2's last trial (if round 2 made no iteration,
 *            round 1's), a level-1 edge with the chi2 of round 1's, every edge with the depth at the final estimate.
 * There is no "no fixed KeyFrame" return and no second-camera arm in this routine.  Every point is a vertex; one without an edge
 * returns its input.  *stop_flag (may be NULL) is read where g2o calls terminate() and once between the rounds (:3718).
 * edge_level1 [n_edges]: the levels after round 1 (all zero when round 2 was skipped); edge_outlier [n_edges]: vToErase.
 * status: 0 optimised; 2 the flag was set before optimize (:3709-3711), or rose before the first iteration (the reference would
 * classify errors it never computed): every output repeats its input, no flag is set; 3 the flag was up after round 1: no levels,
 * no round 2, the flags of the one classification.  active_keyframes / active_points: the vertices of round 2's problem.
 * More free KeyFrames than the capacity, or no room for the reduced system: MSORB_E_CAPACITY, nothing launched, nothing written.
 * MSORB_E_ARG as msorb_local_ba.  Two calls on the same input return the same bits.  Re-entrant like msorb_local_ba.
 * msorb_welding_ba_stage_ms: msorb_local_ba_stage_ms for the calling thread's last call, both rounds added. */
typedef struct msorb_welding_ba_round {
    int iterations, trials, rejected_trials, reserved;
    double chi2_initial, chi2_final, lambda_final;
} msorb_welding_ba_round;
typedef struct msorb_welding_ba_result {
    int status, n_level1, n_outliers, active_keyframes, active_points, reserved;
    msorb_welding_ba_round round[2];
} msorb_welding_ba_result;
/* Test hook: the calling thread's msorb_welding_ba calls fn(user, round, where, iteration, trials) at every place where it is about
 * to read *stop_flag after the entry check, so a test raises its flag at a chosen poll and the call takes that arm every time.
 * round: 0 / 1.  where: before an iteration (sparse_optimizer.cpp:376), after a rejected trial whose rho is negative
 * (levenberg.cpp:149), between the rounds (Optimizer.cc:3718).  iteration: the iteration about to begin or under way; trials: the
 * round's trials so far.  fn = NULL (the default) removes it.  No other entry calls it. */
#define MSORB_WELDING_POLL_ITERATION 0
#define MSORB_WELDING_POLL_REJECTED 1
#define MSORB_WELDING_POLL_BETWEEN 2
typedef void (*msorb_welding_ba_poll_fn)(void* user, int round, int where, int iteration, int trials);
void msorb_debug_welding_ba_poll_hook(msorb_welding_ba_poll_fn fn, void* user);
int msorb_welding_ba_capacity(void);                   /* free KeyFrames: msorb_bundle_adjustment_capacity() */
int msorb_welding_ba_stage_ms(float ms[4]);
int msorb_welding_ba(int device, int n_kf, const msorb_ba_keyframe* kfs, int n_points, const float* pos_w,
                     int n_edges, const int* edge_kf, const int* edge_point, const float* xy, const float* u_right,
                     const float* inv_sigma2, const volatile int* stop_flag,
                     float* kf_qt_out, double* kf_qt_d, float* pos_out, double* pos_d, uint8_t* edge_level1, uint8_t* edge_outlier,
                     msorb_welding_ba_result* r, float* elapsed_ms);

/* Optimizer::PoseOptimization for a frame with a second camera (the arm src/Optimizer.cc:870-931, e.g. a KannalaBrandt8 stereo rig)
 * and for a one-camera frame whose camera is not a pinhole, on the device: the routine of msorb_pose_optimization_batch (the four
 * rounds, g2o's Levenberg loop, the classifications, in double, ONE launch) over the edges EdgeSE3ProjectXYZOnlyPose (left camera:
 * obs - pCamera->project(T.map(Xw)), Jacobian -projectJac * SE3deriv) and EdgeSE3ProjectXYZOnlyPoseToBody (right camera, through
 * mTrl; OptimizableTypes.{h,cpp}).  Every edge has two rows, deltaMono and chi2Mono: the reference cannot build a stereo edge in
 * this arm.  Appended to ABI 6002: MSORB_ABI_VERSION stays 6002.  msorb_pose_result is the one of msorb_pose_optimization_batch.
 * A camera is GeometricCamera::mvParameters as floats: type 0 = Pinhole (fx fy cx cy in p[0..3]), 1 = KannalaBrandt8 (fx fy cx cy
 * k0 k1 k2 k3 in p[0..7]).  KannalaBrandt8::project(Vector3d) takes theta and psi through float sqrtf / atan2f
 * (KannalaBrandt8.cpp:48-49): the device narrows a double atan2 once where glibc runs its float algorithm, so a projection may
 * differ from the reference's by one float ulp of theta or psi now and then (DESIGN.md has the measured share).  A point exactly
 * on a KannalaBrandt8 camera's optical axis gives the reference 0/0 in projectJac; that case is not restated.
 * With n_cameras == 1 and a pinhole the result equals msorb_pose_optimization_batch with every u_right < 0, bit for bit. */
typedef struct msorb_camera_model { int type; float p[8]; } msorb_camera_model;
typedef struct msorb_pose_rig_problem {
    float q[4], t[3];            /* pFrame->GetPose(), the LEFT camera: unit quaternion x,y,z,w + translation */
    int n_cameras;               /* 1 or 2 */
    msorb_camera_model cam[2];   /* mpCamera, mpCamera2 */
    float q_rl[4], t_rl[3];      /* pFrame->GetRelativePoseTrl(); read when n_cameras == 2 */
    int n;                       /* observations */
} msorb_pose_rig_problem;
/* Observations up to which a problem is held in registers; a larger one walks global memory (same additions, same result). */
int msorb_pose_optimization_rig_capacity(void);
/* As msorb_pose_optimization_batch (one upload, one launch, one read-back; obs_offset, xy, inv_sigma2, pos_w, outlier_out, results,
 * elapsed_ms and n < 3 as there), with camera [per observation: 0 = seen by the left camera (i < Nleft, mvKeys), 1 = by the right
 * (mvKeysRight)] in place of u_right.  Left and right observations may come in any order and are summed in the order given.
 * MSORB_E_INVALID, with nothing launched: a camera type other than 0 / 1, n_cameras outside {1, 2}, camera[i] == 1 (or above) in
 * a problem with one camera.  Two calls on the same input return the same bits.  Re-entrant per calling thread. */
int msorb_pose_optimization_rig_batch(int device, int n_problems, const msorb_pose_rig_problem* problems, const int* obs_offset,
                                      const float* xy, const uint8_t* camera, const float* inv_sigma2, const float* pos_w,
                                      uint8_t* outlier_out, msorb_pose_result* results, float* elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* MSORB_H */
