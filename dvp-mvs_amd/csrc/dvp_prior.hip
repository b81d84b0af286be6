// dvp_prior.hip — the monocular-depth plane prior of a FIRST_INIT pass on the device: dep/<id>.dmb + sfm/<id>.txt -> the context's
// planes (APD.cpp:1210-1424), what host/prior.cpp's BuildPlanePrior computes pixel by pixel.  The arithmetic lives in
// dvp_prior.hpp; the sequential part — the sparse points' ratios, the Delaunay triangulation, the triangle list — stays on the host
// (dvp_prior_mid.hpp) ahead of the kernels.  A fixed sequence of launches whatever the inputs hold:
//   host     points, triangulation, skip rules -> the triangle list; the triangles' row counts and their prefix sum
//   upload   the dep map as read, the list, the prefix sum
//            (memset)                  owner map = -1
//            dvp_prior_sequences       one lane per triangle: its counter sequence s_0 = 0, s_{k+1} = fl32(s_k + step)
//            dvp_prior_owners          one wave per (triangle, row), the row's columns over its lanes: atomicMax(owner[pixel], triangle)
//            dvp_prior_rates           per dep-map pixel: the middle rate, or calculateZ of the owning triangle        (binary64)
//            dvp_prior_depth           per working-size pixel: (255 - raw) / rate at the pixel RescaleMatToTargetSize reads
//            dvp_prior_planes          PlanesFromDepth with the context's reference camera -> the context's planes
// The owner map makes the result independent of the order in which the sweep's items run: of several triangles that reach a pixel
// the host loop keeps the last one in list order, here the largest index wins.
#include <hip/hip_runtime.h>

#include <chrono>

#include "dvp_prior_mid.hpp"
#include "dvp_prior_run.h"

namespace dvpprior {

// (the counts come from the host, which sized the buffer with them: a lane writes its triangle's slots and no other)
__global__ void __launch_bounds__(256) dvp_prior_sequences(const Tri* __restrict__ tris, const unsigned* __restrict__ row_off, unsigned T, float* __restrict__ seq) {
	const unsigned t = blockIdx.x * 256u + threadIdx.x;
	if (t >= T) return;
	const unsigned first = row_off[t], n = row_off[t + 1] - first;
	const float step = tris[t].step;
	float s = 0;
	for (unsigned k = 0; k < n; ++k) {
		seq[first + k] = s;
		s = seq_next(s, step);
	}
}

// Work-groups of four waves, one (triangle, row) item per wave.  The items are numbered across the triangles by the prefix sum
// of the row counts, so a triangle of 3000 rows and one of 3 cost their own share.
__global__ void __launch_bounds__(256) dvp_prior_owners(const Tri* __restrict__ tris, const unsigned* __restrict__ row_off, unsigned T, const float* __restrict__ seq,
                                                        int cols, int rows, int32_t* __restrict__ owner) {
	const unsigned item = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (T == 0 || item >= row_off[T]) return;
	unsigned lo = 0, hi = T;   // the triangle: the last t with row_off[t] <= item
	while (hi - lo > 1) {
		const unsigned mid = (lo + hi) / 2;
		if (row_off[mid] <= item) lo = mid; else hi = mid;
	}
	const unsigned first = row_off[lo], n = row_off[lo + 1] - first;
	const Tri t = tris[lo];
	const float p = seq[first + (item - first)];
	// s is non-decreasing and 1.0 - p <= 1.0: the columns of a row are a prefix of the triangle's sequence
	for (unsigned j = lane; j < n; j += 64) {
		const float q = seq[first + j];
		if (!column_exists(p, q)) break;
		const int x = sweep_coord(p, q, t.x1, t.x2, t.x3), y = sweep_coord(p, q, t.y1, t.y2, t.y3);
		// (with all corners inside the map and weights that are not negative no pixel lies outside; the host loop has no such test)
		if (x >= 0 && x < cols && y >= 0 && y < rows) atomicMax(&owner[(size_t)y * cols + x], (int32_t)lo);
	}
}

__global__ void __launch_bounds__(256) dvp_prior_rates(const Tri* __restrict__ tris, const int32_t* __restrict__ owner, float middle_rate, int cols, int rows, float* __restrict__ rate) {
	const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
	if (x >= cols || y >= rows) return;
	const size_t i = (size_t)y * cols + x;
	rate[i] = rate_at(tris, owner[i], middle_rate, x, y);
}

__global__ void __launch_bounds__(256) dvp_prior_depth(const float* __restrict__ raw, const float* __restrict__ rate, int cols, int rows, float scale_x, float scale_y, int W, int H,
                                                       float* __restrict__ depth) {
	const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
	if (c >= W || r >= H) return;
	depth[(size_t)r * W + c] = working_depth(raw, rate, cols, rows, scale_x, scale_y, r, c);
}

__global__ void __launch_bounds__(256) dvp_prior_planes(const float* __restrict__ depth, int W, int H, const DvpCamera* __restrict__ cam, P4* __restrict__ planes) {
	const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
	if (x >= W || y >= H) return;
	planes[(size_t)y * W + x] = plane_at(depth, W, H, cam->K, cam->R, x, y);
}

static dim3 blocks2d(int W, int H) { return dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)); }

// carves the pool; grows it when it is too small (after a wait: queued work may still use the old block)
static int reserve(hipStream_t stream, Scratch& s, size_t dep_pixels, size_t work_pixels, size_t triangles, size_t sweep_rows) {
	dvpmem::Carve c;
	const size_t o_raw = c.take(dep_pixels * 4), o_owner = c.take(dep_pixels * 4), o_rate = c.take(dep_pixels * 4), o_depth = c.take(work_pixels * 4),
	             o_tris = c.take((triangles + 1) * sizeof(Tri)), o_off = c.take((triangles + 1) * 4), o_seq = c.take((sweep_rows + 1) * 4);
	if (s.pool.reserve(c.total, stream)) return 1;
	uint8_t* b = s.pool.as<uint8_t>();
	s.raw = (float*)(b + o_raw); s.owner = (int32_t*)(b + o_owner); s.rate = (float*)(b + o_rate); s.depth = (float*)(b + o_depth);
	s.tris = (Tri*)(b + o_tris); s.row_off = (unsigned*)(b + o_off); s.seq = (float*)(b + o_seq);
	return 0;
}

int run(hipStream_t stream, Scratch& s, const float* dep_raw, int cols, int rows, const float* xy, const float* xyz, int num_points, const DvpCamera* file_camera,
        const DvpCamera* cam, int W, int H, void* planes, int* status, const char** error) {
	using clock = std::chrono::steady_clock;
	auto fail = [error](const char* what) { *error = what; return 1; };
	*status = 1;
	if ((long long)cols * rows > 0x7fffffffLL) return fail("dvp_plane_prior: the dep map has more than 2^31 - 1 pixels");

	// ---- the host part
	const clock::time_point t0 = clock::now();
	float middle_rate = 0;
	if (!dvppriormid::PriorTriangles(dep_raw, cols, rows, xy, xyz, num_points > 0 ? (size_t)num_points : 0, file_camera->K, file_camera->R, file_camera->t, &middle_rate, &s.tris_host))
		return 0;   // status 1: nothing was touched, the last run's maps included
	s.ran = false;
	const size_t T = s.tris_host.size();
	s.row_off_host.resize(T + 1);
	unsigned long long total = 0;
	for (size_t t = 0; t < T; ++t) {
		s.row_off_host[t] = (unsigned)total;
		total += seq_count(s.tris_host[t].step);
		if (total > 0x7fffffffULL) return fail("dvp_plane_prior: too many sweep rows");
	}
	s.row_off_host[T] = (unsigned)total;
	const size_t Ld = (size_t)cols * rows, Lw = (size_t)W * H;
	if (reserve(stream, s, Ld, Lw, T, (size_t)total)) return fail("dvp_plane_prior: out of device memory");
	s.cols = cols; s.rows = rows; s.W = W; s.H = H;
	s.triangles = (long long)T;
	s.sweep_rows = (long long)total;

	// ---- the uploads
	const clock::time_point t1 = clock::now();
	if (hipMemcpyAsync(s.raw, dep_raw, Ld * 4, hipMemcpyHostToDevice, stream) != hipSuccess ||
	    (T && hipMemcpyAsync(s.tris, s.tris_host.data(), T * sizeof(Tri), hipMemcpyHostToDevice, stream) != hipSuccess) ||
	    hipMemcpyAsync(s.row_off, s.row_off_host.data(), (T + 1) * 4, hipMemcpyHostToDevice, stream) != hipSuccess ||
	    hipMemsetAsync(s.owner, 0xFF, Ld * 4, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
		(void)hipGetLastError();
		return fail("dvp_plane_prior: upload failed");
	}

	// ---- the kernels
	const clock::time_point t2 = clock::now();
	const unsigned tri_blocks = (unsigned)((T + 255) / 256 > 0 ? (T + 255) / 256 : 1), row_blocks = (unsigned)((total + 3) / 4 > 0 ? (total + 3) / 4 : 1);
	hipLaunchKernelGGL(dvp_prior_sequences, dim3(tri_blocks), dim3(256), 0, stream, s.tris, s.row_off, (unsigned)T, s.seq);
	hipLaunchKernelGGL(dvp_prior_owners, dim3(row_blocks), dim3(256), 0, stream, s.tris, s.row_off, (unsigned)T, s.seq, cols, rows, s.owner);
	hipLaunchKernelGGL(dvp_prior_rates, blocks2d(cols, rows), dim3(64, 4), 0, stream, s.tris, s.owner, middle_rate, cols, rows, s.rate);
	// RescaleMatToTargetSize's ratios (APD.cpp:1777-1778); equal sizes give 1 and the identity, where the host skips the call
	const float scale_x = W / static_cast<float>(cols), scale_y = H / static_cast<float>(rows);
	hipLaunchKernelGGL(dvp_prior_depth, blocks2d(W, H), dim3(64, 4), 0, stream, s.raw, s.rate, cols, rows, scale_x, scale_y, W, H, s.depth);
	hipLaunchKernelGGL(dvp_prior_planes, blocks2d(W, H), dim3(64, 4), 0, stream, s.depth, W, H, cam, (P4*)planes);
	if (hipGetLastError() != hipSuccess) return fail("dvp_plane_prior: launch failed");
	if (hipStreamSynchronize(stream) != hipSuccess) { (void)hipGetLastError(); return fail("dvp_plane_prior: the kernels failed"); }
	const clock::time_point t3 = clock::now();
	s.ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
	s.ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
	s.ms[2] = std::chrono::duration<double, std::milli>(t3 - t2).count();
	s.ran = true;
	*status = 0;
	return 0;
}

int stage(hipStream_t stream, Scratch& s, int which, void* dst, const char** error) {
	auto fail = [error](const char* what) { *error = what; return 1; };
	if (!s.ran) return fail("dvp_plane_prior_stage: no dvp_plane_prior with status 0 has finished on this context");
	const size_t Ld = (size_t)s.cols * s.rows, Lw = (size_t)s.W * s.H;
	const void* src = nullptr;
	size_t bytes = 0;
	switch (which) {
	case DVP_PRIOR_STAGE_OWNER: src = s.owner; bytes = Ld * 4; break;
	case DVP_PRIOR_STAGE_RATE: src = s.rate; bytes = Ld * 4; break;
	case DVP_PRIOR_STAGE_DEPTH: src = s.depth; bytes = Lw * 4; break;
	default: return fail("dvp_plane_prior_stage: no such stage (DVP_PRIOR_STAGE_*)");
	}
	if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
		(void)hipGetLastError();
		return fail("dvp_plane_prior_stage: download failed");
	}
	return 0;
}

}   // namespace dvpprior
