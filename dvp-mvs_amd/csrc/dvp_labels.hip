// dvp_labels.hip — the label prior on the device: EdgeSegment(scale, image, 1) (APD.cpp:348-401, 437-499), the low-texture
// segmentation the driver's helper threads ran per view (host/labels.cpp).  The arithmetic lives in dvp_labels.hpp, the components
// are dvp_viewclean's (tile labelling in LDS, seam merge, size roll-up on a one-plane word map), the Hough transform stays on the
// host (dvp_labels_mid.hpp) between two device halves.  A fixed sequence of launches whatever the image holds:
//   part A   dvp_lab_resize x 2        full -> half -> quarter size bytes
//            dvp_lab_texture           Roberts cross + threshold -> texture bytes + the word map (1 = white)
//            dvp_vc_tiles / _seams / _rollup
//            dvp_lab_regions           root index of a large black component, else -1     -> the host (read-back 1)
//   host     outlines, HoughSegments, draw_line -> a list of quarter-size pixel indices
//   part B   dvp_lab_scatter           255 at the listed pixels of a copy of the texture map
//            dvp_lab_resize            to the level size, re-thresholded
//            dvp_lab_clean             frame clean-up -> cleaned bytes + the word map
//            dvp_vc_tiles / _seams / _rollup
//            dvp_lab_root_sums / _scan_sums / _ranks   exclusive prefix sum over the root flags in three launches: no work-group
//                                      waits for another
//            dvp_lab_final             0 = white, -1 = small, else 1 + rank of the root    -> the host (read-back 2)
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/dvp_mvs.h"
#include "dvp_labels.hpp"
#include "dvp_labels_mid.hpp"
#include "dvp_viewclean_run.h"

namespace dvplab {

// thr < 0: the resized byte; else (byte > thr ? 255 : 0)
__global__ void __launch_bounds__(256) dvp_lab_resize(const uint8_t* __restrict__ src, size_t pitch, int sw, int sh, double sx, double sy, uint8_t* __restrict__ dst, int dw, int dh,
                                                      int thr) {
	const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
	if (x >= dw || y >= dh) return;
	const uint8_t v = resized_byte(src, pitch, sw, sh, sx, sy, x, y);
	dst[(size_t)y * dw + x] = thr < 0 ? v : (v > thr ? (uint8_t)255 : (uint8_t)0);
}

__global__ void __launch_bounds__(256) dvp_lab_texture(const uint8_t* __restrict__ quarter, int W, int H, uint8_t* __restrict__ texture, uint32_t* __restrict__ words) {
	const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
	if (x >= W || y >= H) return;
	const uint8_t t = texture_at(quarter, W, H, x, y);
	const size_t i = (size_t)y * W + x;
	texture[i] = t;
	words[i] = t ? 1u : 0u;
}

__global__ void __launch_bounds__(256) dvp_lab_regions(const uint32_t* __restrict__ words, const unsigned* __restrict__ parent, const unsigned* __restrict__ size, int weak_tex_num,
                                                       int32_t* __restrict__ region, size_t L) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= L) return;
	region[i] = region_at(words, parent, size, weak_tex_num, i);
}

// (every writer stores the same byte)
__global__ void __launch_bounds__(256) dvp_lab_scatter(uint8_t* __restrict__ map, const unsigned* __restrict__ list, size_t count, size_t L) {
	const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= count) return;
	const unsigned i = list[k];
	if (i < L) map[i] = 255;
}

struct WhitePx {
	const uint8_t* map;
	int W;
	__device__ bool operator()(int y, int x) const { return map[(size_t)y * W + x] != 0; }
};
__global__ void __launch_bounds__(256) dvp_lab_clean(const uint8_t* __restrict__ resized, int W, int H, uint8_t* __restrict__ cleaned, uint32_t* __restrict__ words) {
	const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
	if (x >= W || y >= H) return;
	const size_t i = (size_t)y * W + x;
	const bool frame = x == 0 || y == 0 || x == W - 1 || y == H - 1;
	const uint8_t v = frame ? cleaned_at(WhitePx{ resized, W }, x, y, W, H) : resized[i];   // W, H >= 3: columns 1, W - 2 and rows 1, H - 2 exist
	cleaned[i] = v;
	words[i] = v ? 1u : 0u;
}

// ---- the numbering: rank[root] = roots before it in raster order.  A work-group owns SCAN_BLOCK consecutive pixels, a lane four
constexpr int kScanLanes = SCAN_BLOCK / 4;
// exclusive prefix of v over the work-group's lanes; *total = the sum over all of them
__device__ unsigned block_exclusive(unsigned v, unsigned* lds, unsigned* total) {
	const int t = threadIdx.x;
	lds[t] = v;
	__syncthreads();
	for (int d = 1; d < kScanLanes; d <<= 1) {
		const unsigned add = t >= d ? lds[t - d] : 0u;
		__syncthreads();
		lds[t] += add;
		__syncthreads();
	}
	const unsigned incl = lds[t];
	*total = lds[kScanLanes - 1];
	__syncthreads();   // (lds is written again by the caller's next round)
	return incl - v;
}
__device__ unsigned roots_of_lane(const uint32_t* words, const unsigned* parent, size_t first, size_t L, unsigned flags[4]) {
	unsigned n = 0;
	for (int k = 0; k < 4; ++k) {
		flags[k] = first + k < L ? is_root(words, parent, first + k) : 0u;
		n += flags[k];
	}
	return n;
}
__global__ void __launch_bounds__(kScanLanes) dvp_lab_root_sums(const uint32_t* __restrict__ words, const unsigned* __restrict__ parent, size_t L, unsigned* __restrict__ sums) {
	__shared__ unsigned lds[kScanLanes];
	unsigned flags[4], total;
	const unsigned n = roots_of_lane(words, parent, (size_t)blockIdx.x * SCAN_BLOCK + (size_t)threadIdx.x * 4, L, flags);
	(void)block_exclusive(n, lds, &total);
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one work-group: sums[b] becomes the number of roots in the blocks before b
__global__ void __launch_bounds__(kScanLanes) dvp_lab_scan_sums(unsigned* sums, unsigned blocks) {
	__shared__ unsigned lds[kScanLanes];
	unsigned carry = 0;
	for (unsigned base = 0; base < blocks; base += kScanLanes) {
		const unsigned b = base + threadIdx.x;
		const unsigned v = b < blocks ? sums[b] : 0u;
		unsigned total;
		const unsigned before = block_exclusive(v, lds, &total);
		if (b < blocks) sums[b] = carry + before;
		carry += total;
	}
}
__global__ void __launch_bounds__(kScanLanes) dvp_lab_ranks(const uint32_t* __restrict__ words, const unsigned* __restrict__ parent, size_t L, const unsigned* __restrict__ sums,
                                                            unsigned* __restrict__ rank) {
	__shared__ unsigned lds[kScanLanes];
	unsigned flags[4], total;
	const size_t first = (size_t)blockIdx.x * SCAN_BLOCK + (size_t)threadIdx.x * 4;
	const unsigned n = roots_of_lane(words, parent, first, L, flags);
	unsigned before = sums[blockIdx.x] + block_exclusive(n, lds, &total);
	for (int k = 0; k < 4; ++k)
		if (flags[k]) rank[first + k] = before++;
}
__global__ void __launch_bounds__(256) dvp_lab_final(const uint32_t* __restrict__ words, const unsigned* __restrict__ parent, const unsigned* __restrict__ size,
                                                     const unsigned* __restrict__ rank, int weak_tex_num, int32_t* __restrict__ label, size_t L) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= L) return;
	label[i] = label_at(words, parent, size, rank, weak_tex_num, i);
}

static dim3 blocks2d(int W, int H) { return dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)); }
static unsigned blocks1d(size_t n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

}   // namespace dvplab

using dvplab::Geometry;

// ---- the job: its own stream, one device allocation that grows and is kept -------------------------------------------------------
struct dvp_labels {
	int device = 0;
	hipStream_t stream = nullptr;
	dvpmem::DevBlock pool;
	dvpvc::Scratch vc;
	// the pool's parts for the geometry of the last run
	uint8_t *src = nullptr, *half = nullptr, *quarter = nullptr, *texture = nullptr, *lines = nullptr, *resized = nullptr, *cleaned = nullptr;
	int32_t *region = nullptr, *label = nullptr;
	uint32_t* words = nullptr;
	unsigned *list = nullptr, *rank = nullptr, *sums = nullptr;
	Geometry g{};
	bool ran = false;
	std::vector<int32_t> region_host;
	std::vector<uint8_t> drawn;
	std::vector<unsigned> drawn_list;
	double ms[3] = { 0, 0, 0 };           // part A, the host middle, part B of the last run
	long long regions = 0, points = 0;    // large regions with an outline, outline points over all of them
};

static thread_local dvpmem::CallError t_labels_error;
static int labels_fail(const char* who, const char* what) { return t_labels_error.fail(who, what); }

extern "C" const char* dvp_labels_last_error(void) { return t_labels_error.c_str(); }

extern "C" int dvp_labels_sizes(int width, int height, int scale, int* quarter_cols, int* quarter_rows, int* level_cols, int* level_rows, int* weak_tex_num) {
	t_labels_error.clear();
	if (width < 1 || height < 1 || scale < 0 || scale > 10 || (long long)width * height > 0x7fffffffLL) return labels_fail("dvp_labels_sizes", "bad image geometry or scale (0 ... 10)");
	const Geometry g = dvplab::geometry(width, height, scale);
	if (quarter_cols) *quarter_cols = g.qw;
	if (quarter_rows) *quarter_rows = g.qh;
	if (level_cols) *level_cols = g.lw;
	if (level_rows) *level_rows = g.lh;
	if (weak_tex_num) *weak_tex_num = g.weak_tex_num;
	return 0;
}

extern "C" int dvp_labels_create(int device, dvp_labels** out) {
	t_labels_error.clear();
	if (!out) return labels_fail("dvp_labels_create", "the output pointer is required");
	*out = nullptr;
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return labels_fail("dvp_labels_create", "hipSetDevice failed"); }
	dvp_labels* job = new dvp_labels();
	job->device = device;
	if (hipStreamCreateWithFlags(&job->stream, hipStreamNonBlocking) != hipSuccess) {
		(void)hipGetLastError();
		delete job;
		return labels_fail("dvp_labels_create", "hipStreamCreate failed");
	}
	*out = job;
	return 0;
}

extern "C" int dvp_labels_destroy(dvp_labels* job) {
	t_labels_error.clear();
	if (!job) return 0;
	(void)hipSetDevice(job->device);
	(void)hipStreamSynchronize(job->stream);
	(void)hipStreamDestroy(job->stream);
	delete job;   // frees the pool and the components' scratch
	return 0;
}

// carves the pool for g; grows it when it is too small.  No wait before a regrow: the job's stream is idle here, every
// dvp_labels_run and dvp_labels_stage ends in a hipStreamSynchronize.
static int labels_reserve(dvp_labels* job, const Geometry& g) {
	const size_t Lf = (size_t)g.W * g.H, Lh = (size_t)g.hw * g.hh, Lq = (size_t)g.qw * g.qh, Ll = (size_t)g.lw * g.lh, Lm = Lq > Ll ? Lq : Ll;
	const size_t blocks = (Ll + dvplab::SCAN_BLOCK - 1) / dvplab::SCAN_BLOCK;
	dvpmem::Carve c;
	const size_t o_src = c.take(Lf), o_half = c.take(Lh), o_quarter = c.take(Lq), o_texture = c.take(Lq), o_lines = c.take(Lq), o_region = c.take(Lq * 4),
	             o_words = c.take(Lm * 4), o_list = c.take(Lq * 4), o_resized = c.take(Ll), o_cleaned = c.take(Ll), o_rank = c.take(Ll * 4), o_label = c.take(Ll * 4),
	             o_sums = c.take((blocks + 1) * 4);
	if (job->pool.reserve(c.total) || dvpvc::scratch_reserve(job->vc, Lm, 1)) return 1;
	uint8_t* b = job->pool.as<uint8_t>();
	job->src = b + o_src; job->half = b + o_half; job->quarter = b + o_quarter; job->texture = b + o_texture; job->lines = b + o_lines;
	job->region = (int32_t*)(b + o_region); job->words = (uint32_t*)(b + o_words); job->list = (unsigned*)(b + o_list);
	job->resized = b + o_resized; job->cleaned = b + o_cleaned; job->rank = (unsigned*)(b + o_rank); job->label = (int32_t*)(b + o_label); job->sums = (unsigned*)(b + o_sums);
	return 0;
}

static void labels_resize(dvp_labels* job, const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh, int thr) {
	hipLaunchKernelGGL(dvplab::dvp_lab_resize, dvplab::blocks2d(dw, dh), dim3(64, 4), 0, job->stream, src, (size_t)sw, sw, sh, (double)sw / dw, (double)sh / dh, dst, dw, dh, thr);
}

extern "C" int dvp_labels_run(dvp_labels* job, const uint8_t* grey, int width, int height, long long pitch_bytes, int scale, int32_t* label_out) {
	using namespace dvplab;
	using clock = std::chrono::steady_clock;
	const char* who = "dvp_labels_run";
	t_labels_error.clear();
	if (!job || !grey || !label_out) return labels_fail(who, "the job, the image and the output pointer are required");
	if (scale < 0 || scale > 10) return labels_fail(who, "scale must be 0 ... 10");
	if (width < 1 || height < 1 || (long long)width * height > 0x7fffffffLL || pitch_bytes < width) return labels_fail(who, "bad image geometry (pitch < width, or more than 2^31 - 1 pixels)");
	const Geometry g = geometry(width, height, scale);
	if (g.qw < 3 || g.qh < 3) return labels_fail(who, "the quarter-size map must be at least 3 x 3 (width / 2 / 2, height / 2 / 2)");
	if (g.lw < 3 || g.lh < 3) return labels_fail(who, "the level-size map must be at least 3 x 3 (the frame clean-up reads columns 1, W - 2 and rows 1, H - 2)");
	if ((long long)g.lw * g.lh > 0x7fffffffLL) return labels_fail(who, "bad image geometry");
	if (hipSetDevice(job->device) != hipSuccess) { (void)hipGetLastError(); return labels_fail(who, "hipSetDevice failed"); }
	job->ran = false;
	if (labels_reserve(job, g)) return labels_fail(who, "out of device memory");
	job->g = g;
	hipStream_t st = job->stream;
	const size_t Lq = (size_t)g.qw * g.qh, Ll = (size_t)g.lw * g.lh;
	unsigned* parent = job->vc.words();

	// ---- part A
	const clock::time_point t0 = clock::now();
	if (hipMemcpy2DAsync(job->src, (size_t)width, grey, (size_t)pitch_bytes, (size_t)width, (size_t)height, hipMemcpyHostToDevice, st) != hipSuccess) return labels_fail(who, "upload failed");
	labels_resize(job, job->src, g.W, g.H, job->half, g.hw, g.hh, -1);
	labels_resize(job, job->half, g.hw, g.hh, job->quarter, g.qw, g.qh, -1);
	hipLaunchKernelGGL(dvp_lab_texture, blocks2d(g.qw, g.qh), dim3(64, 4), 0, st, job->quarter, g.qw, g.qh, job->texture, job->words);
	if (hipGetLastError() != hipSuccess || dvpvc::launch_components(st, job->vc, job->words, g.qw, g.qh, 1)) return labels_fail(who, "launch failed");
	hipLaunchKernelGGL(dvp_lab_regions, dim3(blocks1d(Lq)), dim3(256), 0, st, job->words, parent, parent + Lq, g.weak_tex_num, job->region, Lq);
	if (hipGetLastError() != hipSuccess) return labels_fail(who, "launch failed");
	job->region_host.resize(Lq);
	if (hipMemcpyAsync(job->region_host.data(), job->region, Lq * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
		(void)hipGetLastError();
		return labels_fail(who, "the region map could not be fetched");
	}

	// ---- the host middle: the drawn pixels, each once
	const clock::time_point t1 = clock::now();
	job->drawn.assign(Lq, 0);
	job->drawn_list.clear();
	size_t points = 0;
	const int qw = g.qw;
	job->regions = (long long)dvplabmid::DrawRegionLines(job->region_host.data(), g.qw, g.qh, g.unit, [job, qw](int x, int y) {
		const size_t i = (size_t)y * qw + x;
		if (!job->drawn[i]) { job->drawn[i] = 1; job->drawn_list.push_back((unsigned)i); }
	}, &points);
	job->points = (long long)points;

	// ---- part B
	const clock::time_point t2 = clock::now();
	const size_t count = job->drawn_list.size();
	if (hipMemcpyAsync(job->lines, job->texture, Lq, hipMemcpyDeviceToDevice, st) != hipSuccess ||
	    (count && hipMemcpyAsync(job->list, job->drawn_list.data(), count * 4, hipMemcpyHostToDevice, st) != hipSuccess)) {
		(void)hipGetLastError();
		return labels_fail(who, "upload failed");
	}
	hipLaunchKernelGGL(dvp_lab_scatter, dim3(blocks1d(count)), dim3(256), 0, st, job->lines, job->list, count, Lq);
	labels_resize(job, job->lines, g.qw, g.qh, job->resized, g.lw, g.lh, ROBERTS_THRESHOLD);
	hipLaunchKernelGGL(dvp_lab_clean, blocks2d(g.lw, g.lh), dim3(64, 4), 0, st, job->resized, g.lw, g.lh, job->cleaned, job->words);
	if (hipGetLastError() != hipSuccess || dvpvc::launch_components(st, job->vc, job->words, g.lw, g.lh, 1)) return labels_fail(who, "launch failed");
	const unsigned blocks = (unsigned)((Ll + SCAN_BLOCK - 1) / SCAN_BLOCK);
	hipLaunchKernelGGL(dvp_lab_root_sums, dim3(blocks), dim3(kScanLanes), 0, st, job->words, parent, Ll, job->sums);
	hipLaunchKernelGGL(dvp_lab_scan_sums, dim3(1), dim3(kScanLanes), 0, st, job->sums, blocks);
	hipLaunchKernelGGL(dvp_lab_ranks, dim3(blocks), dim3(kScanLanes), 0, st, job->words, parent, Ll, job->sums, job->rank);
	hipLaunchKernelGGL(dvp_lab_final, dim3(blocks1d(Ll)), dim3(256), 0, st, job->words, parent, parent + Ll, job->rank, g.weak_tex_num, job->label, Ll);
	if (hipGetLastError() != hipSuccess) return labels_fail(who, "launch failed");
	if (hipMemcpyAsync(label_out, job->label, Ll * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
		(void)hipGetLastError();
		return labels_fail(who, "the label map could not be fetched");
	}
	const clock::time_point t3 = clock::now();
	job->ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
	job->ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
	job->ms[2] = std::chrono::duration<double, std::milli>(t3 - t2).count();
	job->ran = true;
	return 0;
}

extern "C" int dvp_labels_stage(dvp_labels* job, int which, void* dst) {
	const char* who = "dvp_labels_stage";
	t_labels_error.clear();
	if (!job || !dst) return labels_fail(who, "the job and the destination are required");
	if (!job->ran) return labels_fail(who, "no run has finished on this job");
	const size_t Lq = (size_t)job->g.qw * job->g.qh, Ll = (size_t)job->g.lw * job->g.lh;
	const void* src = nullptr;
	size_t bytes = 0;
	switch (which) {
	case DVP_LABEL_STAGE_QUARTER: src = job->quarter; bytes = Lq; break;
	case DVP_LABEL_STAGE_TEXTURE: src = job->texture; bytes = Lq; break;
	case DVP_LABEL_STAGE_REGION: src = job->region; bytes = Lq * 4; break;
	case DVP_LABEL_STAGE_LINES: src = job->lines; bytes = Lq; break;
	case DVP_LABEL_STAGE_RESIZED: src = job->resized; bytes = Ll; break;
	case DVP_LABEL_STAGE_CLEANED: src = job->cleaned; bytes = Ll; break;
	default: return labels_fail(who, "no such stage (DVP_LABEL_STAGE_*)");
	}
	if (hipSetDevice(job->device) != hipSuccess) { (void)hipGetLastError(); return labels_fail(who, "hipSetDevice failed"); }
	if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, job->stream) != hipSuccess || hipStreamSynchronize(job->stream) != hipSuccess) {
		(void)hipGetLastError();
		return labels_fail(who, "download failed");
	}
	return 0;
}

extern "C" int dvp_labels_timings(const dvp_labels* job, double* ms, long long* counts) {
	t_labels_error.clear();
	if (!job || !job->ran) return labels_fail("dvp_labels_timings", "no run has finished on this job");
	if (ms) for (int k = 0; k < 3; ++k) ms[k] = job->ms[k];
	if (counts) { counts[0] = job->regions; counts[1] = job->points; }
	return 0;
}

extern "C" int dvp_label_map(int device, const uint8_t* grey, int width, int height, long long pitch_bytes, int scale, int32_t* label_out) {
	dvp_labels* job = nullptr;
	if (dvp_labels_create(device, &job)) return 1;
	const int rc = dvp_labels_run(job, grey, width, height, pitch_bytes, scale, label_out);
	const dvpmem::CallError message = t_labels_error;
	(void)dvp_labels_destroy(job);
	t_labels_error = message;
	return rc;
}
