/* dvp_mvs.h — C ABI of the MI355X PatchMatch engine (libdvp_mvs_hip.so).
 *
 * Drop-in boundary for the per-view depth/normal path of ZhenlongYuan/DVP-MVS: these entry
 * points are what the reference's `class APD` methods (APD.h:94-199) do with the CUDA runtime
 * — allocate/upload (APD::CudaSpaceInitialization, APD.cpp:1497-1613), bundle the buffers
 * (APD::SetDataPassHelperInCuda, APD.cpp:1670-1704; DataPassHelper, APD.h:60-92), run the kernel
 * sequence (APD::RunPatchMatch, APD.cu:4406-4532) and copy the results back (APD.cu:4525-4530).
 * Plain pointers and sizes only; POD layouts are the reference's (main.h:58-67, 86-112).
 * All functions return 0 on success, non-zero on error (dvp_last_error() gives the text); the
 * C++ mirror of `class APD` (dvp-mvs_amd/host/APD.h) turns non-zero into the reference's
 * print-and-exit (CudaSafeCall, APD.cpp:943-951).
 * One context == one reference view on one device/stream; contexts are independent (no global
 * state), so one process can own several and N processes can own one GPU each.
 */
#ifndef DVP_MVS_H_
#define DVP_MVS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVP_MAX_IMAGES 32        /* main.h:39 */
#define DVP_NEIGHBOUR_NUM 12     /* main.h:40 */
#define DVP_EDGE_NEIGH_NUM 8     /* main.h:43 */
#define DVP_LAB_BOUNDARY_NUM 8   /* main.h:44 */

/* struct Camera, main.h:58-67 (112 bytes). x_cam = R X + t, c = -R^T t. */
typedef struct DvpCamera {
	float K[9];
	float R[9];
	float t[3];
	float c[3];
	int32_t height;
	int32_t width;
	float depth_min;
	float depth_max;
} DvpCamera;

/* enum RunState, main.h:74-78 ; enum PixelState, main.h:80-84 */
enum { DVP_FIRST_INIT = 0, DVP_REFINE_INIT = 1, DVP_REFINE_ITER = 2 };
enum { DVP_WEAK = 0, DVP_STRONG = 1, DVP_UNKNOWN = 2 };

/* struct PatchMatchParams, main.h:86-112 (76 bytes; C++ bool == uint8_t) */
typedef struct DvpParams {
	int32_t max_iterations;
	int32_t num_images;
	float sigma_spatial;
	float sigma_color;
	int32_t top_k;
	float depth_min;
	float depth_max;
	uint8_t geom_consistency;
	int32_t strong_radius;
	int32_t strong_increment;
	int32_t weak_radius;
	int32_t weak_increment;
	uint8_t use_APD;
	uint8_t use_edge;
	uint8_t use_limit;
	uint8_t use_label;
	uint8_t use_detail;
	uint8_t use_radius;
	int32_t weak_peak_radius;
	int32_t rotate_time;
	float ransac_threshold;
	float geom_factor;
	int32_t state;
} DvpParams;

typedef struct dvp_ctx dvp_ctx;

/* Kernel launches of APD::RunPatchMatch, one id per launch site (APD.cu:4430-4505). */
enum {
	DVP_ST_GEN_EDGE_INFORM = 0,      /* GenEdgeInform          APD.cu:4433 */
	DVP_ST_FIND_NEAREST_STRONG = 1,  /* FindNearestStrongPoint APD.cu:4445 */
	DVP_ST_GEN_NEIGHBOURS = 2,       /* GenNeighbours          APD.cu:4448 */
	DVP_ST_NEIGHBOUR_UPDATE = 3,     /* NeigbourUpdate         APD.cu:4451 */
	DVP_ST_RANDOM_INIT = 4,          /* RandomInitialization   APD.cu:4475 */
	DVP_ST_STRONG_UPDATE = 5,        /* Black/RedPixelUpdateStrong  APD.cu:4479-4481 */
	DVP_ST_RANSAC_FIT = 6,           /* RANSACToGetFitPlane    APD.cu:4484 */
	DVP_ST_WEAK_UPDATE = 7,          /* Black/RedPixelUpdateWeak    APD.cu:4487-4489 */
	DVP_ST_GET_DEPTH_NORMAL = 8,     /* GetDepthandNormal      APD.cu:4494 */
	DVP_ST_FILTER_STRONG = 9,        /* Black/RedPixelFilterStrong  APD.cu:4497-4499 */
	DVP_ST_DEPTH_TO_WEAK = 10,       /* DepthToWeak            APD.cu:4502 */
	DVP_ST_LOCAL_REFINE = 11,        /* LocalRefine            APD.cu:4505 */
	DVP_ST_LAUNCHABLE = 12,          /* ids below this one are launch sites accepted by dvp_run_stage */
	DVP_ST_STRONG_PREP = 12,         /* timing bucket only: the pre-launch snapshot copies and the sample-search
	                                    launch issued by every DVP_ST_STRONG_UPDATE (DvpTimings) */
	DVP_ST_COUNT = 13
};

/* Device buffers (DataPassHelper members, APD.h:60-92) addressable by dvp_download_buffer /
 * dvp_upload_buffer. */
enum {
	DVP_BUF_PLANES = 0,              /* float4 per pixel   plane_hypotheses_cuda */
	DVP_BUF_COSTS = 1,               /* float              costs_cuda */
	DVP_BUF_SELECTED_VIEWS = 2,      /* uint32             selected_views_cuda */
	DVP_BUF_VIEW_WEIGHT = 3,         /* uint8 x 32         view_weight_cuda */
	DVP_BUF_WEAK_INFO = 4,           /* uint8              weak_info_cuda */
	DVP_BUF_WEAK_RELIABLE = 5,       /* uint8              weak_reliable_cuda */
	DVP_BUF_WEAK_NEAREST_STRONG = 6, /* short2             weak_nearest_strong */
	DVP_BUF_NEIGHBOURS_MAP = 7,      /* int32              neighbours_map_cuda */
	DVP_BUF_NEIGHBOURS = 8,          /* short2 x 12 per WEAK pixel   neighbours_cuda */
	DVP_BUF_FIT_PLANES = 9,          /* float4             fit_plane_hypotheses_cuda */
	DVP_BUF_CANDIDATE = 10,          /* short2 x 8 x (num_images-1) per pixel  candidate_cuda */
	DVP_BUF_EDGE = 11,               /* uint8              edge_cuda */
	DVP_BUF_EDGE_NEIGH = 12,         /* short2 x 8         edge_neigh_cuda */
	DVP_BUF_LABEL = 13,              /* int32              label_cuda */
	DVP_BUF_LABEL_BOUNDARY = 14,     /* short2 x 8 per WEAK pixel    label_boundary_cuda */
	DVP_BUF_COMPLEX = 15,            /* float per WEAK pixel         complex_cuda */
	DVP_BUF_RADIUS = 16,             /* int32              radius_cuda */
	DVP_BUF_COUNT = 17
};

/* Per-launch-site timing, measured with HIP events on the engine's own stream. */
typedef struct DvpTimings {
	double stage_ms[DVP_ST_COUNT];      /* accumulated kernel time per launch site */
	int32_t stage_launches[DVP_ST_COUNT];
	double iter_loop_ms;                /* the iteration loop, APD.cu:4478-4492 */
	double total_ms;                    /* whole dvp_run_patchmatch */
	uint64_t ncc_evals[DVP_ST_COUNT];   /* bilateral-NCC evaluations per launch site (only when
	                                       dvp_set_profiling(ctx, 1): counting build) */
} DvpTimings;

/* ---- lifetime (APD::APD / ~APD, APD.cpp:984-1043; cudaSetDevice, main.cpp:430-434) ---------- */
/* limits: 2 <= num_images <= 32 (APD.cpp:1083-1086), width, height <= 32767 (short2 pixel coordinates),
 * (width+4 rounded up to 64) * (height+4) * 8 bytes < 4 GiB (32-bit offsets into a row-pair plane) */
int dvp_ctx_create(int device, int width, int height, int num_images, dvp_ctx** out);
int dvp_ctx_destroy(dvp_ctx* ctx);
const char* dvp_last_error(const dvp_ctx* ctx);   /* ctx may be NULL: last create error */

/* ---- uploads (APD::CudaSpaceInitialization, APD.cpp:1497-1613) ------------------------------- */
/* images[i]: host pointer, row-major float32, `pitch_floats` elements per row (>= width);
 * replaces cudaMemcpy2DToArray + cudaCreateTextureObject (APD.cpp:1501-1517). */
int dvp_upload_images(dvp_ctx* ctx, const float* const* images, int pitch_floats);
/* depth maps of ref + src views for geom_consistency (APD.cpp:1522-1545) */
int dvp_upload_depths(dvp_ctx* ctx, const float* const* depths, int pitch_floats);
/* same, from device memory already resident on ctx's device (e.g. an RCCL broadcast buffer):
 * images/depths are copied device-to-device on the engine's stream. */
int dvp_upload_images_device(dvp_ctx* ctx, const float* const* dev_images, int pitch_floats);
int dvp_upload_depths_device(dvp_ctx* ctx, const float* const* dev_depths, int pitch_floats);
int dvp_upload_cameras(dvp_ctx* ctx, const DvpCamera* cams, int n);            /* APD.cpp:1549-1550 */
/* per-pixel input state; any pointer may be NULL (keeps the current/default content):
 * planes float4 (world normal, depth) APD.cpp:1566-1567 · selected_views APD.cpp:1560-1561 ·
 * weak_info APD.cpp:1595-1596 (also rebuilds neighbours_map/weak_count, APD.cpp:1182-1193) ·
 * edge APD.cpp:1577-1578 · label APD.cpp:1585-1586 · radius APD.cpp:1590-1591. */
int dvp_upload_state(dvp_ctx* ctx, const float* planes_xyzw, const uint32_t* selected_views,
                     const uint8_t* weak_info, const uint8_t* edge, const int32_t* label,
                     const int32_t* radius);
/* The same per-pixel input state for a REFINE_INIT pass whose previous maps come from the COARSER pyramid level
 * (src_w x src_h): replaces the five host-side RescaleMatToTargetSize calls of APD::InuputInitialization /
 * SupportInitialization (APD.cpp:1176-1180, 1440-1449, 1656-1659; the function itself APD.cpp:1773-1795, nearest
 * neighbour, row index / width ratio and column index / height ratio as the source has it), the plane assembly
 * (APD.cpp:1450-1456) and the radius rule for UNKNOWN pixels (APD.cpp:1660-1666) by one kernel on the maps at their own
 * size.  depth, normal_xyz (3 floats per pixel) and selected_views are required; weak_info NULL = every pixel STRONG
 * (APD.cpp:1196-1204); radius NULL = radius map untouched; edge / label are full-size maps as in dvp_upload_state. */
int dvp_upload_state_rescaled(dvp_ctx* ctx, int src_w, int src_h, const float* depth, const float* normal_xyz,
                              const uint32_t* selected_views, const uint8_t* weak_info, const int32_t* radius,
                              int radius_fallback, const uint8_t* edge, const int32_t* label);
/* device-side reset to the state a freshly constructed APD has before a FIRST_INIT pass without
 * prior: planes = 0 (out of range -> random init, APD.cu:1289-1291), selected_views = 0, every
 * pixel STRONG (APD.cpp:1196-1204), radius = strong_radius (APD.cpp:1649-1653), fit planes = 0
 * (APD.cpp:1571); edge/label maps are kept.  Lets one context process consecutive views without
 * host round trips. */
int dvp_reset_state(dvp_ctx* ctx);
/* device-side snapshot of the per-pixel input state (planes, selected_views, weak_info, radius) and
 * its restore (pass-internal buffers return to their freshly-uploaded content): re-running a pass
 * from identical inputs without re-uploading — what a fresh APD per view per pass (main.cpp:273,
 * APD.cpp:984-987) gives the reference for free. */
int dvp_save_state(dvp_ctx* ctx);
int dvp_restore_state(dvp_ctx* ctx);
/* Optional buffers of the context ahead of their first use — what a driver's helper thread calls on the context it prepares
 * for the next pyramid level, so that no multi-GB allocation lands inside a view's launches (the reference allocates everything in
 * CudaSpaceInitialization, APD.cpp:1497-1613).  flags: bit 0 = the split strong update's cost block, bit 1 = the view-compacted
 * DepthToWeak / LocalRefine passes' buffers, bit 2 = the binary16 image planes of format 2 (dvp_image_format: a context for a
 * down-sampled pyramid level), bit 3 = the scratch and output maps of dvp_edge_map_begin (8 + 1 bytes per pixel), bit 4 = the scratch of dvp_set_view_cleanup
 * (8 bytes per pixel and source view); weak_pixels > 0: the weak update's anchor table and hand-over buffers for that many
 * WEAK pixels.  Never required: every launch site (and dvp_upload_images*) allocates what it lacks. */
int dvp_ctx_reserve(dvp_ctx* ctx, int weak_pixels, int flags);
int dvp_set_params(dvp_ctx* ctx, const DvpParams* params);                     /* APD.cpp:1607-1608 */
/* The reference seeds cuRAND with clock64() (APD.cu:1270); here the seed is explicit. */
int dvp_set_seed(dvp_ctx* ctx, uint64_t seed);
/* 0 = CUDA-texture-like 8-bit interpolation weights (default), 1 = exact fractions */
int dvp_set_sampler(dvp_ctx* ctx, int sampler);
int dvp_set_profiling(dvp_ctx* ctx, int count_evals);
/* Image planes the gather-bound kernels read after the last dvp_upload_images*: 0 = the float planes,
 * 1 = byte planes (kept besides the float planes when every texel of every image is an integer in
 * [0, 255]: images decoded from 8-bit files at their native size, APD.cpp:1057-1069), 2 = binary16
 * planes (kept when the set is not 8-bit exact but every texel is finite, in [0, 255] and exact in
 * binary16: power-of-two down-sampled levels of 8-bit images, whose texels are multiples of 0.25).
 * Same values in every format, so results do not depend on it.  DVP_NO_IMAGES8 in the environment
 * forces 0 for every set; DVP_NO_IMAGES16 turns 2 into 0 and leaves 1 alone. */
int dvp_image_format(const dvp_ctx* ctx);
/* The form the context's strong update takes: the view bracket of the split form's decision kernel (4, 6, 8, 10, 12, 16; 32 = the
 * streaming kernel for up to 31 views, DVP_STRONG_WIDE=1 in the environment at dvp_ctx_create: 17 ... 31 source views, =2: every
 * count), or 0 for a monolithic kernel.  The split form's cost buffers are allocated by the first strong update (or by
 * dvp_ctx_reserve, bit 0): from then on a context they did not fit reports 0; before, the answer assumes that they fit.
 * Same results in every form. */
int dvp_strong_update_form(const dvp_ctx* ctx);

/* ---- run (APD::RunPatchMatch, APD.cu:4406-4532) ---------------------------------------------- */
int dvp_run_patchmatch(dvp_ctx* ctx);
/* one launch site of the sequence; colour: 0 = Black*, 1 = Red* for the half launches (weak update also 2 = both colours as
 * one launch site, which is how dvp_run_patchmatch issues it: the two launches commute) */
int dvp_run_stage(dvp_ctx* ctx, int stage, int iter, int colour);
int dvp_synchronize(dvp_ctx* ctx);

/* ---- results (cudaMemcpy D2H, APD.cu:4525-4530; getters APD.cpp:1706-1748) ------------------- */
/* any pointer may be NULL. planes: (world normal xyz, depth w) per pixel. */
int dvp_download_state(dvp_ctx* ctx, float* planes_xyzw, uint32_t* selected_views,
                       uint8_t* weak_info, int32_t* radius);
/* The same results in the form the reference's driver stores them (ProcessProblem, main.cpp:300-309, which loops over
 * GetPlaneHypothesis): depth map = plane.w where depth_min <= w <= depth_max, else 0 and the pixel's state becomes
 * UNKNOWN (in the downloaded copy; the device state is untouched); normal map = 3 floats per pixel.  depth, normal_xyz
 * and weak_info are required. */
int dvp_download_maps(dvp_ctx* ctx, float* depth, float* normal_xyz, uint32_t* selected_views,
                      uint8_t* weak_info, int32_t* radius);
/* dvp_download_maps in two steps, for a driver that puts the next view on this context while the maps of the last one still
 * travel (the reference downloads synchronously, APD.cpp:1616-1640; a 25-Mpx view is 640 MB = 27 ms of PCIe time between 900 ms
 * of kernels).  _begin forms the maps in a staging buffer on the device — and, if depth_device_copy is not NULL, copies the
 * depth map to that DEVICE buffer (width * height floats: the resident map other views read as a source) — and returns when
 * the device is done with that; the context may then be reset, uploaded to and run again.  _finish copies the staged maps to
 * the host on a stream of its own and may be called from another thread; the next _begin (and dvp_ctx_destroy) waits for it. */
int dvp_download_maps_begin(dvp_ctx* ctx, float* depth_device_copy);
int dvp_download_maps_finish(dvp_ctx* ctx, float* depth, float* normal_xyz, uint32_t* selected_views,
                             uint8_t* weak_info, int32_t* radius);
long long dvp_buffer_bytes(dvp_ctx* ctx, int buffer);
int dvp_download_buffer(dvp_ctx* ctx, int buffer, void* dst);
int dvp_upload_buffer(dvp_ctx* ctx, int buffer, const void* src);
int dvp_weak_count(dvp_ctx* ctx);
int dvp_get_timings(dvp_ctx* ctx, DvpTimings* out);
int dvp_reset_timings(dvp_ctx* ctx);

/* ---- roofline micro-benchmark / known-answer tests ------------------------------------------- */
/* n (pixel, plane) pairs -> out[n * (num_images-1)] = ComputeMultiViewCostVectorOld
 * (APD.cu:1207-1216).  px = {x0,y0,x1,y1,...}; planes = camera-frame (nx,ny,nz,d) per pair.
 * Host pointers.  If kernel_ms != NULL it receives the kernel's HIP-event time. */
int dvp_eval_cost_vectors(dvp_ctx* ctx, const int32_t* px, const float* planes, int n, float* out,
                          float* kernel_ms);
/* device-resident variant for benchmarking: same computation on every pixel of the image with
 * plane = current plane_hypotheses (camera frame), `repeat` launches; returns the mean kernel ms */
/* sha256 of the kernel sources the library was built from (tools/csrc_hash.py), + the extra flags of a variant build */
const char* dvp_build_id(void);
int dvp_bench_cost_kernel(dvp_ctx* ctx, int repeat, float* mean_kernel_ms, uint64_t* evals_per_launch);

/* ---- depth-map fusion (RunFusion, APD.cpp:1809-1960) on the device ------------------------------
 * Replaces the body of the reference's host loop over views / pixels / sources: the geometric tests of every (pixel, source)
 * pair (Get3DPointonWorld + ProjectCamera + GetAngle, APD.cpp:1893-1931), the consistency vote (:1926-1929), the acceptance
 * (:1934) and the claims on the witnesses (`masks[...]`, :1888, 1911, 1942) — same points, same order, same bits as the
 * sequential scan (dvp-mvs_amd/csrc/dvp_fuse.hip says how the order-dependent claims are resolved in parallel).  The caller
 * keeps what the reference does around it: reading maps / images / cameras (:1836-1871) and writing the .ply (:1955-1958).
 * One job = one scene on one device.  acos / exp are the specified functions of csrc/dvp_fuse_math.hpp. */
typedef struct dvp_fuse dvp_fuse;
int dvp_fuse_create(int device, int num_views, dvp_fuse** out);
int dvp_fuse_destroy(dvp_fuse* job);
const char* dvp_fuse_last_error(const dvp_fuse* job);        /* job == NULL: the error of a failed dvp_fuse_create */
/* the maps of view slot `view` (host pointers, copied): camera with the intrinsics ALREADY rescaled to the maps' size
 * (RescaleImageAndCamera, APD.cpp:1750-1771), depth [rows*cols], normal [rows*cols*3], weak_info [rows*cols] or NULL
 * (every pixel STRONG), bgr [rows*cols*3] (the colour image at the maps' size), block [rows*cols] or NULL
 * (blocks/mask_<id>.jpg: reference pixels below 128 are skipped, APD.cpp:1885-1887) */
int dvp_fuse_set_view(dvp_fuse* job, int view, const DvpCamera* cam, int cols, int rows, const float* depth,
                      const float* normal_xyz, const uint8_t* weak_info, const uint8_t* bgr, const uint8_t* block);
/* one iteration of the reference's outer loop (APD.cpp:1874): view slot `view` scanned against the source slots `src`
 * (pair.txt order, sources without maps left out); accepted points are appended to the cloud in scan order */
int dvp_fuse_view(dvp_fuse* job, int view, const int* src, int num_src);
/* ... and of RunFusion_TAT_Intermediate (advanced = 0, APD.cpp:1962-2130) / RunFusion_TAT_advanced (advanced = 1,
 * APD.cpp:2132-2279): `src` holds ALL sources of the view in pair.txt order, -1 for a source without maps */
int dvp_fuse_view_graded(dvp_fuse* job, int view, const int* src, int num_src, int advanced);
/* the consistency mask of view slot `view`, what the mesher (dvp_mesh_*) integrates: mask_out[p] = 1 iff the pixel is a reference
 * pixel (depth > 0, block mask >= 128) and at least min_views of the source slots `src` (all with maps, any number) pass the three
 * tests of the scan (reprojection < 2 px, relative depth < 1 %, normals < 0.174533 rad), claims ignored; room for rows*cols bytes.  It
 * reads no claim and writes none: the cloud of the dvp_fuse_view calls before and after it is what it is without the call. */
int dvp_fuse_consistency(dvp_fuse* job, int view, const int* src, int num_src, int min_views, uint8_t* mask_out);
long long dvp_fuse_count(const dvp_fuse* job);               /* points so far */
/* dvp_fuse_count() records of six floats — x y z b g r, struct PointList (main.h:69-72) — in scan order */
int dvp_fuse_download(dvp_fuse* job, float* points);
/* statistics of the last dvp_fuse_view: rounds of the parallel claim resolution, pixels left to the sequential finish */
int dvp_fuse_last_rounds(const dvp_fuse* job, int* rounds, int* rest);

/* ---- preview images and baseline JPEG (ShowDepthMap / ShowNormalMap / ShowWeakImage + cv::imwrite, APD.cpp:694-812) ----
 * JPEG files as cv::imwrite has libjpeg write them — JFIF 1.01, quality scaling of the Annex K tables (baseline), YCbCr 4:2:0
 * (3 channels) or grey (1), the accurate integer DCT, the standard Huffman tables — plus a DRI segment and RST markers every
 * `restart_mcus` MCUs (an MCU is 16x16 pixels in colour, 8x8 in grey), which is what lets the device code the segments in
 * parallel.  Decoded, such a file gives the pixels of the same image written without restart markers. */
enum { DVP_PREVIEW_DEPTH = 1, DVP_PREVIEW_NORMAL = 2, DVP_PREVIEW_WEAK = 4 };
/* an upper bound of the file size of any image of that geometry (any quality, any restart interval); -1 for bad arguments */
long long dvp_jpeg_bound(int width, int height, int channels);
/* Stateless, host in / host out: pixels are `channels` (1, or 3 in BGR order) bytes per pixel, `pitch_bytes` per row;
 * quality 1..100 (the reference's imwrite: 95); restart_mcus 1..65535, 0 = the engine's choice.  Writes the file
 * to dst and its size to *bytes; if capacity is too small, *bytes still receives the size and the call fails. */
int dvp_jpeg_encode(int device, const uint8_t* pixels, int width, int height, int channels, long long pitch_bytes, int quality,
                    int restart_mcus, uint8_t* dst, long long capacity, long long* bytes);
const char* dvp_jpeg_last_error(void);   /* the calling thread's last dvp_jpeg_encode error */
/* Renders the previews named by `kinds` (DVP_PREVIEW_* bits) from the context's current planes and weak map — the maps the
 * driver stores: depth = plane.w inside [params.depth_min, depth_max], else 0, state UNKNOWN where it is outside — and encodes
 * them (quality 1..100, the engine's restart interval) on the context's stream; returns after one wait for the encoded sizes.
 * _finish (the file: header, data, EOI) and _pixels (the BGR image before encoding, width * height * 3 bytes) may be called
 * from any thread until the next dvp_preview_begin.  A driver begins the previews right after dvp_download_maps_begin and
 * fetches them in the job that calls dvp_download_maps_finish, before that call: the next view's dvp_download_maps_begin then
 * cannot come before the fetch.  Allocation failures are returned as errors (dvp_last_error). */
int dvp_preview_begin(dvp_ctx* ctx, int kinds, int quality);
int dvp_preview_finish(dvp_ctx* ctx, int kind, uint8_t* dst, long long capacity, long long* bytes);
int dvp_preview_pixels(dvp_ctx* ctx, int kind, uint8_t* bgr);

/* ---- the depth-edge prior (EdgeSegment(scale, image, mode 0, use_canny), APD.cpp:404-466) on the device -------------------------
 * The median-adaptive Canny whose result fills DVP_BUF_EDGE: median of the grey histogram over bins 0..254 (-1 if more than half
 * of the pixels are 255), thresholds (int)((1 - 0.67f) * median) and median, cv::Canny's rules for 8-bit input with aperture 3 and
 * L2gradient (Sobel with replicated border, squared thresholds, sector suppression with the fixed-point tan 22.5 test, hysteresis
 * over 8-connected candidates), 255 / 0, then the frame fix-ups of APD.cpp:452-463.  Integer arithmetic: the map is the same on
 * every device and equal to the host mirror's EdgeSegment byte for byte.  Widths and heights below 3 are rejected (the fix-ups
 * read columns 1, W - 2 and rows 1, H - 2).  The number of launches does not depend on the image. */
/* Stateless, host in / host out: grey is width x height bytes, `pitch_bytes` per row; edge_out receives width * height bytes. */
int dvp_canny_edge_map(int device, const uint8_t* grey, int width, int height, long long pitch_bytes, uint8_t* edge_out);
/* The hysteresis step alone: map3 holds 0 = candidate, 1 = nothing, 2 = strong per pixel (width * height bytes); edge_out
 * receives 255 where a pixel is strong or a candidate 8-connected through candidates to a strong pixel, else 0; no fix-ups. */
int dvp_edge_hysteresis(int device, const uint8_t* map3, int width, int height, uint8_t* edge_out);
const char* dvp_edge_last_error(void);   /* the calling thread's last dvp_canny_edge_map / dvp_edge_hysteresis error */
/* The edge map of the context's image 0 — grey byte = the texel rounded to nearest (ties to even) and saturated, what the
 * reference's convertTo(CV_8UC1) gives (main.cpp:205-214) — on the context's stream, without a host wait; install != 0 also
 * writes it to DVP_BUF_EDGE, as dvp_upload_state(..., edge, ...) of the same map would.  An error before the first
 * dvp_upload_images*.  _finish copies the map (width * height bytes) to the host and may be called from another thread once
 * _begin has returned.  The context keeps the maps of the last two _begin calls: _finish returns the oldest one not fetched
 * yet, so a driver may begin the next view's map on a context before the last view's background job has fetched its own. */
int dvp_edge_map_begin(dvp_ctx* ctx, int install);
int dvp_edge_map_finish(dvp_ctx* ctx, uint8_t* edge);

/* ---- the visibility-mask clean-up of ProcessProblem (main.cpp:311-363) on the device ----------------------------------------------
 * For every bit i < num_src of the selected-view words: the 4-connected components (no diagonal contact) of the pixels whose bit i
 * is clear are formed, and  out bit i = in bit i | (the pixel's component has fewer than min_region pixels); a component of exactly
 * min_region pixels stays clear, min_region <= 0 changes no bit below num_src.  Bits >= num_src are 0 in out; num_src = 0 gives
 * zeros.  The reference's driver passes min_region = 20 * (8 / scale_size)^2 in integer arithmetic.  Integer and exact: equal to
 * the host mirror's Connect + fill loop word for word.  Four launches whatever the words hold. */
/* Stateless, host in / host out: views and out are width * height words (out may be views); width, height >= 1; num_src outside
 * 0 ... 32 is an error.  Scratch: 8 * num_src bytes per pixel, for the duration of the call. */
int dvp_clean_selected_views(int device, const uint32_t* views, int width, int height, int num_src, int min_region, uint32_t* out);
const char* dvp_viewclean_last_error(void);   /* the calling thread's last dvp_clean_selected_views error */
/* enable != 0: from now on dvp_download_maps_begin (and with it dvp_download_maps) cleans the STAGED copy of the selected-view words
 * with these arguments, on the context's stream before its wait: _finish hands out the cleaned words, DVP_BUF_SELECTED_VIEWS keeps
 * the raw ones (as weak_info keeps the states the UNKNOWN rule changes in the staged copy).  Off by default; enable = 0 restores
 * exactly what dvp_download_maps_begin did before.  The scratch (8 * num_src bytes per pixel) is allocated at the first use or by
 * dvp_ctx_reserve bit 4 and freed with the context. */
int dvp_set_view_cleanup(dvp_ctx* ctx, int enable, int num_src, int min_region);

/* ---- the label prior (EdgeSegment(scale, image, mode 1), APD.cpp:348-401, 437-499) on the device ----------------------------------
 * The low-texture segmentation whose result fills DVP_BUF_LABEL, from the FULL-size grey image whatever the level: two bilinear
 * halvings (cv::resize through float, rounded to nearest even), Roberts cross with the reference's byte cast and threshold 4,
 * 4-connected components of the flat pixels at quarter size; on the host, between the two device halves, the progressive
 * probabilistic Hough transform over the outline of every region of at least weak_tex_num pixels and the lines it finds; then the
 * resize to the level, the threshold again, the frame clean-up, components at level size numbered 1, 2, ... in raster order of
 * their first pixels, 0 = textured, -1 = a region of at most weak_tex_num pixels.  Equal to the host mirror's LabelSegment value
 * for value.  The number of launches does not depend on the image.
 *   quarter size = (width / 2 / 2) x (height / 2 / 2)                        (integer divisions)
 *   level size   = round(width * f) x round(height * f), float f = 1 / 2^scale  (halves away from zero)
 *   weak_tex_num = (int)(1.0 * width * height / (1024 << scale << scale))
 * dvp_labels_sizes returns them (NULL pointers are skipped).  scale outside 0 ... 10, a quarter or level map below 3 x 3,
 * pitch_bytes < width, null pointers are errors with a message (dvp_labels_last_error). */
typedef struct dvp_labels dvp_labels;
int dvp_labels_sizes(int width, int height, int scale, int* quarter_cols, int* quarter_rows, int* level_cols, int* level_rows, int* weak_tex_num);
/* A job: its own stream; device scratch that grows on demand and is kept for the next image (about 1.9 bytes per full-size pixel
 * plus 22 per level pixel).  Two jobs may run at the same time from two threads; one job serves one thread at a time. */
int dvp_labels_create(int device, dvp_labels** out);
int dvp_labels_destroy(dvp_labels* job);
/* grey: width x height bytes, `pitch_bytes` per row; label_out receives level cols x level rows int32.  Returns after the map
 * has arrived: the call waits twice, for the region map the host middle reads and for the result. */
int dvp_labels_run(dvp_labels* job, const uint8_t* grey, int width, int height, long long pitch_bytes, int scale, int32_t* label_out);
/* After a run: an intermediate map of it.  QUARTER, TEXTURE, LINES: quarter-size bytes (the grey image; 255 = textured; the same
 * with the lines drawn); REGION: quarter-size int32, the smallest pixel index of the pixel's flat region where that has at least
 * weak_tex_num pixels, else -1; RESIZED, CLEANED: level-size bytes before and after the frame clean-up. */
enum { DVP_LABEL_STAGE_QUARTER = 0, DVP_LABEL_STAGE_TEXTURE = 1, DVP_LABEL_STAGE_REGION = 2, DVP_LABEL_STAGE_LINES = 3, DVP_LABEL_STAGE_RESIZED = 4, DVP_LABEL_STAGE_CLEANED = 5 };
int dvp_labels_stage(dvp_labels* job, int which, void* dst);
/* After a run: ms[3] = wall time of the first device half (upload to region map), the host middle, the second device half;
 * counts[2] = regions with an outline, outline points over all of them.  NULL pointers are skipped. */
int dvp_labels_timings(const dvp_labels* job, double* ms, long long* counts);
/* One-shot: create, run, destroy. */
int dvp_label_map(int device, const uint8_t* grey, int width, int height, long long pitch_bytes, int scale, int32_t* label_out);
const char* dvp_labels_last_error(void);   /* the calling thread's last dvp_labels_* / dvp_label_map error */

/* ---- level images made on the device from the decoded 8-bit files (load_image, host/APD.cpp; APD.cpp:1057-1131) -----------------
 * A store keeps decoded grey images on one device, 1 byte per pixel, under ids the caller chooses.  A level image is a function of
 * such an image: the bytes lie at the origin of a pad_w x pad_h canvas (zero beyond the image, cropped beyond the canvas: what the
 * reference does to a source of another size than its reference image), the canvas becomes float, and cv::resize(INTER_LINEAR)
 * takes it to the level size — source coordinate (float)((d + 0.5) * s - 0.5) with s = (double)pad_n / level_n, floor, the
 * second tap clamped to the canvas, the horizontal blend on two rows and then the vertical one, each p * (1.f - a) + q * a in
 * binary32 without fused operations.  Equal sizes give the bytes as floats.  Equal to the host mirror's load_image value for value,
 * so a caller needs no cv::resize of its own to feed a context.
 * The store is locked internally: uploads from several contexts and threads and dvp_images_level calls are reads and run side by
 * side, and a dvp_images_put of another id may run beside them.  Dropping an id (or destroying the store) while an upload or a
 * level call uses it is the caller's error. */
typedef struct dvp_images dvp_images;
int dvp_images_create(int device, dvp_images** out);
int dvp_images_destroy(dvp_images* store);
/* grey: width x height bytes, `pitch_bytes` per row; copied to the device, returns when the copy is done.  An id already present is
 * an error (dvp_images_drop it first); widths and heights of 1 ... 32767. */
int dvp_images_put(dvp_images* store, int id, const uint8_t* grey, int width, int height, long long pitch_bytes);
int dvp_images_drop(dvp_images* store, int id);                                  /* != 0: not in the store */
int dvp_images_size(const dvp_images* store, int id, int* width, int* height);   /* != 0: not in the store; NULL pointers are skipped */
long long dvp_images_bytes(const dvp_images* store);                             /* device bytes held */
/* One level to the host: host_out receives level_w x level_h floats, dense.  pad_w = pad_h = 0: the image's own size.  Any sizes of
 * 1 ... 32767, up-sampling included. */
int dvp_images_level(dvp_images* store, int id, int pad_w, int pad_h, int level_w, int level_h, float* host_out);
const char* dvp_images_last_error(void);   /* the calling thread's last dvp_images_* error */
/* Fills the context's num_images images with the levels of ids[0 .. num_images-1] at the context's width x height, every image on
 * a pad_w x pad_h canvas: the reference image's original size, which ids[0] must have exactly.  Everything is checked before the
 * context is touched — the store is on the context's device, every id is present, the sizes are valid — so after an error
 * (dvp_last_error) the context still holds its previous images.  Afterwards the context is in the state dvp_upload_images of
 * those float images leaves it in, buffer for buffer and bit for bit, dvp_image_format included. */
int dvp_upload_images_u8(dvp_ctx* ctx, const dvp_images* store, const int* ids, int pad_w, int pad_h);
/* The width x height float image `index` the context holds since its last dvp_upload_images*, `pitch_floats` (>= width) per row. */
int dvp_download_image(dvp_ctx* ctx, int index, float* out, int pitch_floats);

/* ---- the input JPEGs decoded on the device (`apd --decode-on gpu`) -----------------------------------------------------------------
 * A baseline / extended-sequential 8-bit JPEG file (Huffman-coded, one interleaved scan, one or three components) in host memory.
 * The marker parse and the entropy decode run on the host, in the text the host mirror's DecodeJpeg runs: a file it rejects
 * (progressive, a truncated segment, a missing table, a corrupt code, a missing restart marker, sub-sampled luma for one channel)
 * is rejected here with the same message, before any device work.  Dequantisation, the accurate integer inverse DCT, the clamp,
 * the replicated chroma sampling and the JFIF colour equations run on the device; the bytes equal DecodeJpeg's.
 * channels 1: the luma plane (libjpeg's JCS_GRAYSCALE); 3: B, G, R.  `out`: height rows of `pitch_bytes` (>= width * channels).
 * out == NULL: only *width and *height are set, from the frame header, and nothing touches the device.  NULL size pointers are
 * skipped.  Host in, host out; returns when `out` is complete.  A refused allocation reports "out of device memory". */
int dvp_jpeg_decode(int device, const uint8_t* file, long long file_bytes, int channels, uint8_t* out, long long pitch_bytes, int* width, int* height);
/* The luma plane of the file reconstructed straight into the store's slot `id`: what dvp_images_put of the decoded plane leaves —
 * 1 byte per pixel, counted in dvp_images_bytes, an id already present is an error — without a host plane in between.  The plane
 * is copied to the host only when grey_out_or_null is given (height rows of pitch_bytes >= width).  After any error the store is
 * as it was.  Sizes of 1 ... 32767. */
int dvp_jpeg_decode_into_store(dvp_images* store, int id, const uint8_t* file, long long file_bytes, uint8_t* grey_out_or_null, long long pitch_bytes);
/* The calling thread's last successful call of the two above: ms[0] the host part (parse + entropy decode), ms[1] the device part
 * (upload, launches, read-back, wait); counts[0] the bytes of coefficient records and offsets uploaded, counts[1] the 8 x 8 blocks. */
int dvp_jpeg_decode_timings(double* ms, long long* counts);
const char* dvp_jpeg_decode_last_error(void);   /* the calling thread's last error of the three above and of dvp_jpeg_scan_records */
/* `apd --entropy-on gpu`: where the Huffman scan of the two decode calls above runs.  Process-wide; 0 (the default): on the host,
 * every call exactly as described above.  1: the headers are parsed on the host, the file's entropy-coded bytes go up instead of
 * coefficient records, and the records are made on the device (csrc/dvp_jpeg_huff.hip: a lane per 128-byte subsequence, which
 * self-synchronises with its neighbours); they never exist on the host.  A file the device path does not take — fill bytes or
 * another marker inside the scan, no marker after it, a restart-marker count that does not match the frame, a corrupt code, a
 * segment that does not hold exactly its MCUs, a synchronisation that does not settle, a refused allocation — is decoded on the
 * host as with 0: same bytes, same messages.  dvp_jpeg_decode_timings: ms[0] is then the parse and the pre-scan, ms[1] everything
 * on the device; counts[0] the bytes of the records and offsets the device made. */
void dvp_jpeg_set_entropy(int on_device);
/* The calling thread's last dvp_jpeg_decode / dvp_jpeg_decode_into_store / dvp_jpeg_scan_records, 8 numbers: [0] the path — 0 host,
 * 1 device, 2 device, then fell back to the host; [1] segments (the stretches between restart markers); [2] subsequences;
 * [3] chunks of 256 subsequences; [4] the longest synchronisation chain (subsequences one lane decoded in a row); [5] inter-chunk
 * rounds; [6] bytes uploaded for the scan; [7] subsequence decodes of the synchronisation in all ([7] / [2] = mean re-decodes). */
int dvp_jpeg_entropy_stats(long long* counts);
/* 7 numbers, milliseconds of the last device-path call of the calling thread when the process runs with DVP_JPEG_ENTROPY_SERIAL=1
 * (a wait after every phase; else zeros but [0]): pre-scan, upload, synchronisation, census + count, scans, write, reconstruction. */
int dvp_jpeg_entropy_phases(double* ms);
/* The coefficient records of a file's scan in the format of csrc/dvp_jpeg_dec_mid.hpp, from the host's serial scan (on_device 0)
 * or from the device path (1, whatever dvp_jpeg_set_entropy says; dvp_jpeg_entropy_stats tells whether it fell back).  Two calls:
 * with offsets == records == NULL only *components and the word counts per component (3 entries each; 0 for a component that
 * is absent or, with luma_only, not wanted) are written; then offsets[i] and records[i] receive that many uint32 words. */
int dvp_jpeg_scan_records(int device, const uint8_t* file, long long file_bytes, int luma_only, int on_device, int* components, long long* offset_words, long long* record_words,
                          uint32_t** offsets, uint32_t** records);

/* ---- the monocular-depth plane prior of a FIRST_INIT pass (APD.cpp:1210-1424) on the device ---------------------------------------
 * From the relative depth map of dep/<id>.dmb (dep_w x dep_h floats as read, dense) and the sparse points of sfm/<id>.txt
 * (xy: 2 floats per point, the image position; xyz: 3 floats, the world point) to the context's planes (DVP_BUF_PLANES), equal
 * to the host mirror's BuildPlanePrior bit for bit (NaN == NaN): every point is projected with file_camera — the camera as
 * cams/<id>_cam.txt holds it, unscaled — and counts when it lands at 0 < ix < dep_w, 0 < iy < dep_h; its rate is
 * (255 - dep(iy, ix)) over the projected depth; the positions are Delaunay-triangulated (csrc/dvp_prior_mid.hpp, on the host) and
 * the rate map is the barycentric interpolation of the rates inside the triangles, the middle point's rate elsewhere; the metric
 * depth (255 - dep) / rate is taken to the context's size with RescaleMatToTargetSize's index rule; the planes are the
 * finite-difference normals of that map with the context's reference camera (dvp_upload_cameras: an error before it), turned
 * towards the camera and to the world frame, and the depth.  *status = 0: the planes were written; 1: an empty map or no usable
 * point — the planes are untouched.  A following dvp_upload_state(ctx, NULL, ...) keeps the planes.  The number of launches
 * does not depend on the inputs.  Scratch: 12 bytes per dep-map pixel + 4 per context pixel, kept with the context;
 * it grows on demand. */
int dvp_plane_prior(dvp_ctx* ctx, const float* dep_raw, int dep_w, int dep_h, const float* xy, const float* xyz, int num_points,
                    const DvpCamera* file_camera, int* status);
/* After a dvp_plane_prior with status 0: an intermediate map of it.  OWNER: dep_w x dep_h int32, the index (in list order) of the
 * triangle whose value the pixel holds, -1 = none; RATE: dep_w x dep_h floats; DEPTH: the metric depth at the context's size,
 * width x height floats. */
enum { DVP_PRIOR_STAGE_OWNER = 0, DVP_PRIOR_STAGE_RATE = 1, DVP_PRIOR_STAGE_DEPTH = 2 };
int dvp_plane_prior_stage(dvp_ctx* ctx, int which, void* dst);
/* ... and ms[3] = wall time of the host part (points + triangulation), the uploads, the kernels; counts[2] = swept triangles,
 * sweep rows over all of them.  NULL pointers are skipped. */
int dvp_plane_prior_timings(dvp_ctx* ctx, double* ms, long long* counts);

/* ---- `apd --convert-from`: the numeric steps of the reference's colmap2mvsnet.py on the device --------------------------------------
 * The view-selection scores of a COLMAP model (calc_score, colmap2mvsnet.py:280-302).  Image i's observations are
 * obs_point_ids[obs_offsets[i] .. obs_offsets[i + 1]) (obs_offsets: num_images + 1 entries from 0; -1 = no point); centres: 3
 * doubles per image; the points are point_ids[k] with xyz[3 k ..].  score_out: num_images x num_images, symmetric, zero diagonal.
 * For i < j: S = the entries of i's list that are not -1 and occur in j's list (a duplicate in i counts each time); the score is
 * S, or 0 when S > 0 and more than (3 * S) >> 2 of the S angles at the points between the two centres,
 * (180 / pi) * acos(dot / |u| / |v|) in binary64 with the cosine clamped to [-1, 1], are below 1 degree - the element at
 * int(S * 0.75) of the sorted angles is then below 1.  Integer counts, so the matrix does not depend on the order of the work.
 * Errors: num_images outside 1 ... 16384, more than 2^31 - 1 observations or points, a point id that occurs twice, an
 * observation that names a point absent from point_ids.  Host in, host out. */
int dvp_view_scores(int device, int num_images, const long long* obs_offsets, const long long* obs_point_ids, const double* centres, long long num_points,
                    const long long* point_ids, const double* xyz, uint32_t* score_out);
/* The picture the converter writes (colmap2mvsnet.py:462-469): the w x h 8-bit B, G, R picture (`pitch` bytes per row) padded with
 * zeros on the right and bottom to pad_w x pad_h, then cv::resize(INTER_NEAREST) to out_w x out_h:
 * sx = min((int)floor(x * (1.0 / ((double)out_w / pad_w))), pad_w - 1), rows alike.  out: out_h dense rows of 3 * out_w bytes.
 * Sizes of 1 ... 65535.  Host in, host out. */
int dvp_convert_image(int device, const uint8_t* bgr, int w, int h, long long pitch, int pad_w, int pad_h, int out_w, int out_h, uint8_t* out);
const char* dvp_pairs_last_error(void);   /* the calling thread's last error of the two above */

/* ---- `apd --convert-from ... --undistort on`: the reference has no counterpart (colmap2mvsnet.py expects pictures that COLMAP's
 * image_undistorter has made, and keeps fx, fy, cx, cy of whatever model it meets); the project's own definition -----------------
 * The w x h 8-bit B, G, R picture (`pitch` bytes per row) taken with COLMAP camera model `model` (COLMAP's id, 0 ... 10) and
 * `params` (COLMAP's order: f or fx, fy; cx, cy; the distortion parameters) resampled into the pinhole camera with the same
 * fx, fy, cx, cy and the same size.  For output pixel (x, y): u = (x + 0.5 - cx) / fx, v alike; (u', v') = the model's forward
 * distortion of (u, v); sx = fx u' + cx - 0.5, sy alike; both quantised to 1 / 32 pixel, floor(32 s + 0.5), and clamped to
 * [-64, 32 size + 64]; then cv::remap(INTER_LINEAR, BORDER_CONSTANT)'s fixed-point rule: the four taps weighted with the two
 * 5-bit fractions, + 512, >> 10, a tap outside the picture counting as 0, a NaN coordinate giving a zero pixel.  Binary64, one
 * rounding per operator, with the library's own atan for the fisheye models (csrc/dvp_undistort.hpp): the bytes do not depend on
 * the device or on libm.  out: h dense rows of 3 * w bytes.  No output size is chosen and nothing is cropped.
 * Errors: a null pointer, an unknown model, FOV (7), a num_params that is not the model's, sizes outside 1 ... 65535, a pitch
 * below 3 * w.  Host in, host out; safe from several threads. */
int dvp_undistort_image(int device, const uint8_t* bgr, int w, int h, long long pitch, int model, const double* params, int num_params, uint8_t* out);
const char* dvp_undistort_last_error(void);   /* the calling thread's last error of the one above */

/* ---- `apd --evaluate`: a fused cloud scored against a ground-truth cloud; the reference has no counterpart, the definition is the
 * project's own (csrc/dvp_cloudeval.hpp, DESIGN.md "Cloud evaluation") ---------------------------------------------------------------
 * For a query p: m(p) = the minimum over the targets q with three finite coordinates of (dx*dx + dy*dy) + dz*dz, d = p - q, in
 * binary32 with one rounding per operator; d2(p) = m(p) if m(p) <= T*T (binary32 product, T = max_distance or the largest
 * tolerance), else +inf; NaN for a query with a non-finite coordinate; +inf everywhere when no target is finite.  Equal to the
 * brute-force double loop bit for bit, whatever order the device works in.
 * d2_out[i] as defined above for query i against the target cloud; xyz arrays are packed float triples (host pointers) */
int dvp_cloud_distances(int device, const float* query_xyz, long long num_query, const float* target_xyz, long long num_target, float max_distance, float* d2_out);
/* both directions and the counts; within_* hold num_tol entries, used[0] / used[1] the finite-coordinate points of recon / truth;
 * d2_recon / d2_truth may be NULL.  within_recon[k] = the finite-coordinate points of recon with d2 <= t_k * t_k (binary32 product)
 * against truth, within_truth[k] the same with the roles swapped: accuracy(k) = within_recon[k] / used[0], completeness(k) =
 * within_truth[k] / used[1].
 * Errors: a null pointer, a count outside 0 ... 2^31 - 1, more than 2^30 points with finite coordinates in the two clouds together
 * (both functions), num_tol outside 1 ... 8, a tolerance that is not finite and positive or
 * whose square is not a normal binary32 number, tolerances that do not strictly ascend, clouds that extend over more than
 * 2^21 - 2 cells of the largest tolerance along an axis, no device memory.  Host in, host out; safe from several threads. */
int dvp_cloud_evaluate(int device, const float* recon_xyz, long long num_recon, const float* truth_xyz, long long num_truth,
                       const float* tolerances, int num_tol, long long* within_recon, long long* within_truth,
                       long long* used, float* d2_recon, float* d2_truth);
const char* dvp_cloud_last_error(void);   /* the calling thread's last error of the two above */

/* ---- the preparation in front of `apd --evaluate`'s distances (--transform, --crop, --voxel-size); the project's own definition
 * (csrc/dvp_cloudprep.hpp, DESIGN.md "Cloud evaluation"), which follows the steps of the Tanks and Temples protocol and pins to no
 * other library's bits ----------------------------------------------------------------------------------------------------------------
 * Binary64 with one rounding per operator; input order is kept.  (1) A point with a non-finite coordinate is dropped.  (2) transform
 * (16 row-major doubles m, or NULL): x' = ((m00*x + m01*y) + m02*z) + m03, y', z' alike; a point with a non-finite image is dropped.
 * (3) crop (crop_axis w = 0, 1, 2; -1 = none): (u, v) = (1, 2), (0, 2), (0, 1); kept iff axis_min <= p[w] <= axis_max and an odd
 * number of polygon edges (i, j = (i + 1) % n) have (Vi[v] < p[v] && Vj[v] >= p[v]) || (Vj[v] < p[v] && Vi[v] >= p[v]) and
 * Vi[u] + (p[v] - Vi[v]) / (Vj[v] - Vi[v]) * (Vj[u] - Vi[u]) < p[u].  (4) voxel (edge s; 0 = none): per axis o = (minimum over the
 * kept points) - s*0.5, t = (p - o) / s, i = floor(t), q = (uint64)floor((t - i) * 2^32); per voxel Q = the integer sum of q, n the
 * count; centroid o + ((double)i + ((double)Q / (double)n) * 2^-32) * s; one point per voxel, ordered by the voxel's first point.
 * (5) Every output coordinate is rounded to binary32 once.  With no option set the output is the finite input points, bit for bit. */
typedef struct dvp_cloud_prep {
	const double* transform;     /* 16 doubles, row-major, last row exactly 0 0 0 1; NULL = none */
	int crop_axis;               /* 0, 1, 2; -1 = no crop */
	double axis_min, axis_max;   /* both inclusive */
	const double* polygon_xyz;   /* num_polygon vertices of three doubles each */
	int num_polygon;             /* 3 ... 256 */
	double voxel;                /* the voxel's edge; 0 = no down-sampling */
} dvp_cloud_prep;
/* One cloud prepared.  xyz_out has room for num points; first_index_out (may be NULL) likewise: first_index_out[k] is the input
 * index of output point k, for a voxel that of its first point.  counts_out[4] = the points with finite coordinates, those left
 * after the transform, those inside the crop, the output points.
 * Errors: a null pointer, a count outside 0 ... 2^31 - 1, a non-finite matrix entry, a last row other than 0 0 0 1, a crop_axis
 * outside -1 ... 2, fewer than 3 or more than 256 vertices, a non-finite vertex, axis_min > axis_max, a voxel that is negative or not
 * finite, more than 2^30 points to down-sample, a cloud that extends over more than 2^21 - 2 voxels along an axis, no device memory.
 * Host in, host out; safe from several threads. */
int dvp_cloud_prepare(int device, const float* xyz, long long num, const dvp_cloud_prep* prep, float* xyz_out, long long* first_index_out,
                      long long* counts_out);
/* Both clouds prepared, each by its own description, then dvp_cloud_evaluate's definition on the prepared clouds, which stay on the
 * device in between.  used[], d2_recon and d2_truth (room for num_recon / num_truth entries; may be NULL) refer to the prepared
 * points in prepared order; counts_out[8] = the four counts of recon, then of truth.  Errors: those of dvp_cloud_prepare and of
 * dvp_cloud_evaluate. */
int dvp_cloud_evaluate_prepared(int device, const float* recon_xyz, long long num_recon, const dvp_cloud_prep* prep_recon, const float* truth_xyz,
                                long long num_truth, const dvp_cloud_prep* prep_truth, const float* tolerances, int num_tol, long long* within_recon,
                                long long* within_truth, long long* used, float* d2_recon, float* d2_truth, long long* counts_out);
const char* dvp_cloud_prep_last_error(void);   /* the calling thread's last error of the two above */

/* ---- `apd --evaluate --refine-alignment`: point-to-point ICP that refines the matrix which brings the reconstruction onto the ground
 * truth; the project's own definition (csrc/dvp_cloudicp.hpp, DESIGN.md "Cloud evaluation") --------------------------------------------
 * One step's device part.  increment D: 16 row-major doubles, last row exactly 0 0 0 1, NULL = identity.  Per source i: p' = D p in
 * binary64 (the preparation's formula), r = p' rounded to binary32; j(i) = the target that minimises e = (dx*dx + dy*dy) + dz*dz,
 * d = r - q_j, in binary32, the smallest j among equal minima; i corresponds iff e <= max_distance * max_distance (binary32).  A source
 * with a non-finite coordinate or a non-finite r never corresponds.  nearest_out[i] = j(i) and e_out[i] = e for a corresponding
 * source, -1 and +inf for every other (both may be NULL).  sums_out[16] = the sums over the corresponding sources of a = p' - c (3),
 * b = q_j - c (3), a_r * b_c (9, row-major) and e, c = the centre of the targets' bounds; each sum is the balanced pairwise tree over
 * the source indices padded with +0.0 to a power of two, so it is the same bits on any device.  *count_out = the corresponding sources.
 * Errors: a null pointer, a count outside 0 ... 2^31 - 1, a target with a non-finite coordinate, a non-finite increment or a last row
 * other than 0 0 0 1, a max_distance that is not finite and positive or whose binary32 square is not normal, targets that extend
 * over too many cells of max_distance, more than 2^30 sources in the wave form of the search (its table of the sources keeps a slot
 * in 32 bits; the lane form takes 2^31 - 1), more than 2^30 targets, no device memory.  Host in, host out; safe from several threads.
 * The search form (DVP_CLOUD_QUERY=wave|lane, default wave) and the neighbourhood (DVP_CLOUD_ICP_CELLS=27|125, default 27) are read
 * from the environment when a call begins; the result does not depend on either. */
int dvp_cloud_icp_step(int device, const float* src_xyz, long long n_src, const float* tgt_xyz, long long n_tgt, const double* increment, float max_distance,
                       int* nearest_out, float* e_out, double* sums_out, long long* count_out);
typedef struct dvp_icp_stage {
	double voxel;          /* both clouds down-sampled at this edge for the stage; 0 = not */
	double max_distance;   /* correspondences reach this far (rounded to binary32) */
	int max_iterations;    /* 1 ... 1000 */
} dvp_icp_stage;
typedef struct dvp_icp_log {
	int stage, step;       /* stage from 0, step from 1 */
	long long n_src, n;    /* the stage's prepared sources, the corresponding ones of this step (n < 3 ends the stage) */
	double rmse;           /* sqrt(sum of e / n); 0 for n = 0 */
} dvp_icp_log;
/* The stages in order.  M = prep_recon->transform (NULL: identity).  Per stage: src = the reconstruction prepared with transform M,
 * prep_recon's crop and the stage's voxel, tgt = the ground truth prepared with prep_truth's crop and the stage's voxel (the voxel and,
 * for the truth, the transform fields of the descriptions are ignored; a NULL description crops nothing); D = I; up to max_iterations
 * steps, each: dvp_cloud_icp_step's sums of D, one log record, then the stage ends when n < 3 or, from the second step on, when
 * fitness = n / n_src and rmse both changed by less than 1e-6; else D <- E D with E the rigid motion that minimises the squared
 * distances of the correspondences (Horn's quaternion method).  After the stage M <- D M.  transform_out[16] = the final M.  The
 * first log_capacity records are stored, *log_count = their total.  Both raw clouds are uploaded once.
 * Errors: those above and of dvp_cloud_prepare, num_stages outside 1 ... 8, a negative or non-finite voxel, max_iterations outside
 * 1 ... 1000, a prepared ground truth with a point that overflows binary32, more than 2^30 reconstruction points in the wave form.
 * Safe from several threads. */
int dvp_cloud_refine_alignment(int device, const float* recon_xyz, long long n_recon, const float* truth_xyz, long long n_truth, const dvp_cloud_prep* prep_recon,
                               const dvp_cloud_prep* prep_truth, const dvp_icp_stage* stages, int num_stages, double* transform_out, dvp_icp_log* log, int log_capacity,
                               int* log_count);
const char* dvp_cloud_icp_last_error(void);   /* the calling thread's last error of the two above */

/* ---- `apd --evaluate --against-scans`: ETH3D's observed-space accuracy from range maps of the laser scans as their scanners saw them;
 * the project's own definition (csrc/dvp_cloudscan.hpp, DESIGN.md "Cloud evaluation") ---------------------------------------------------
 * A scan: num binary32 points in the scanner's own frame and the 16 row-major doubles that bring them into the scene (all finite, last
 * row exactly 0 0 0 1).  Truth point g = transform * q in binary64 (the preparation's formula), rounded once to binary32; the scanner
 * stands at the translation column rounded to binary32.  cube_size R: a power of two, 16 ... 4096.  Per scan a cube map of 6 R R
 * texels around the scanner: map[t] = the smallest squared range r2 = (dx*dx + dy*dy) + dz*dz (binary32) of the scan's truth points
 * whose direction falls into texel t, +inf for none.  gap of a point p: NaN for a non-finite p, else the maximum over the scans that
 * hold a finite value in p's texel of sqrt(map[t]) - sqrt(r2(p)), -inf if none does: a positive gap says that a scanner measured a
 * surface that far behind p. */
typedef struct dvp_cloud_scan { const float* xyz; long long num; double transform[16]; } dvp_cloud_scan;
/* maps, truth points and gaps of the queries; every output may be NULL.  maps_out: num_scans * 6 R R values of r2, truth_xyz_out: 3
 * floats per scan point, scan after scan.  Errors: a null pointer, num_scans outside 1 ... 64, a cube_size that is no power of two in
 * 16 ... 4096, a negative count, more than 2^31 - 1 scan points together, a non-finite transform or a last row other than 0 0 0 1, no
 * device memory.  Host in, host out; safe from several threads. */
int dvp_cloud_scan_gaps(int device, const dvp_cloud_scan* scans, int num_scans, int cube_size, const float* query_xyz, long long num_query, float* gap_out, float* maps_out,
                        float* truth_xyz_out);
/* The whole evaluation against scans: recon prepared by prep_recon, the truth cloud of the scans by prep_truth (either may be NULL:
 * the finite points as they are), dvp_cloud_evaluate's distances and counts on the prepared clouds, then free_space[k] = the prepared
 * reconstructed points with !(d2 <= t_k * t_k) && gap > t_k; the maps are made from every point of every scan, whatever prep_truth
 * holds.  counts_out[8] as dvp_cloud_evaluate_prepared; d2_recon_out and gap_out (room for num_recon values, may be NULL) per
 * prepared reconstructed point.  Errors: those above, of dvp_cloud_prepare and of dvp_cloud_evaluate. */
int dvp_cloud_evaluate_scans(int device, const float* recon_xyz, long long num_recon, const dvp_cloud_prep* prep_recon, const dvp_cloud_scan* scans, int num_scans,
                             const dvp_cloud_prep* prep_truth, int cube_size, const float* tolerances, int num_tol, long long* within_recon, long long* within_truth,
                             long long* used, long long* free_space, long long* counts_out, float* d2_recon_out, float* gap_out);
const char* dvp_cloud_scan_last_error(void);   /* the calling thread's last error of the two above */

/* ---- a surface from the depth maps: a truncated signed distance volume over a hashed grid of 8 x 8 x 8 blocks and the surface nets of
 * its zero level; the project's own definition (csrc/dvp_mesh.hpp, DESIGN.md 7 "Mesh"), pinned to no library ----------------------------
 * voxel s: the lattice's edge in scene units, sample (i, j, k) at ((float)((double)i * s), ...), indices -2^20 ... 2^20 - 1; truncation
 * tau >= s (at most 64 s); a sample counts from min_weight >= 1 views on.  A view: the camera with the intrinsics of the maps' size,
 * depth [rows*cols], mask [rows*cols] (non-zero = the pixel is used, if its depth is positive), bgr [rows*cols*3]; host pointers, copied.
 * dvp_mesh_build: blocks allocated around every masked pixel, every sample integrated over all views in add_view order, then vertices
 * (one per active cell), their colours and the triangles, in the order of the definition: the bytes of the serial text.  A job may be
 * given more views and built again.  Errors: a null pointer; a non-finite or non-positive voxel; a truncation below the voxel, not
 * finite or beyond 64 voxels; min_weight < 1; a lattice index beyond 21 bits; more vertices than an int face index holds; out of device
 * memory.  Jobs are independent: safe from several threads, one thread per job. */
typedef struct dvp_mesh dvp_mesh;
int dvp_mesh_create(int device, float voxel, float truncation, int min_weight, dvp_mesh** out);
int dvp_mesh_destroy(dvp_mesh* job);
int dvp_mesh_add_view(dvp_mesh* job, const DvpCamera* cam, int cols, int rows, const float* depth, const uint8_t* mask, const uint8_t* bgr);
int dvp_mesh_build(dvp_mesh* job);
/* of the last build, -1 without one */
long long dvp_mesh_block_count(const dvp_mesh* job);
long long dvp_mesh_vertex_count(const dvp_mesh* job);
long long dvp_mesh_face_count(const dvp_mesh* job);
/* vertices: 3 floats x y z each, colours: 3 bytes b g r each, faces: 3 vertex numbers each */
int dvp_mesh_download(dvp_mesh* job, float* vertices, uint8_t* colours, int* faces);
/* the volume behind the last build, every output may be NULL: the blocks' keys ascending, then per block 512 samples (local index
 * lx * 64 + ly * 8 + lz) of SF, W, and the four integers b, g, r sums and their count */
int dvp_mesh_download_volume(dvp_mesh* job, unsigned long long* keys, float* sf, int* w, unsigned* colour_sums);
/* the block table's first size (a power of two, 4 ... 2^32; default: from the masked pixels): a table that fills is doubled and the
 * allocation run again, which gives the same set */
int dvp_mesh_set_table(dvp_mesh* job, long long slots);
/* of the last build: ms[3] = allocation, integration, extraction (wall clock, each ends with a wait), the table's doublings, the
 * job's device memory */
int dvp_mesh_timings(const dvp_mesh* job, double* ms, long long* regrows, long long* bytes);
const char* dvp_mesh_last_error(void);   /* the calling thread's last error of the above */

#ifdef __cplusplus
}
#endif
#endif /* DVP_MVS_H_ */
