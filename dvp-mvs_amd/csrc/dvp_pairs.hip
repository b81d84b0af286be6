// dvp_pairs.hip — the device half of `apd --convert-from`: the view-selection scores of a COLMAP model and the image the converter
// writes.  The arithmetic and the host part (argument checks, the tracks) live in dvp_pairs.hpp.
//   dvp_pairs_count    work-groups of four waves, one track element e per wave; the wave's lanes run over the elements f > e of the
//                      same track: unsigned 32-bit atomicAdd into the upper triangles of cnt and low.  Work is the sum of the
//                      squared track lengths, not N^2 times the list length.
//   dvp_pairs_scores   one lane per matrix entry: the score from the two counts, mirrored, zero on the diagonal
//   dvp_pairs_convert  one lane per output byte, a work-group 256 bytes of one row: consecutive lanes store consecutive bytes
// Indices: an element index is below 2^31 (the host checks the observation count), a matrix index below 2^28 (N <= 16384), a
// picture's byte offset is formed in size_t.
// Device memory: one DevBlock per call, carved; the stream of a call is a StreamScope.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/dvp_mvs.h"
#include "dvp_devmem.hpp"
#include "dvp_pairs.hpp"

namespace dvppairs {

struct AtomicAdd {
	__device__ void operator()(uint32_t* p, uint32_t v) const { atomicAdd(p, v); }
};

__global__ void __launch_bounds__(256) dvp_pairs_count(const Tracks t, uint32_t elements, int N, uint32_t* __restrict__ cnt, uint32_t* __restrict__ low) {
	const uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (e >= elements) return;
	const uint32_t end = t.off[t.point[e] + 1];   // <= elements
	for (uint32_t f = e + 1 + lane; f < end; f += 64) pair_item(t, e, f, N, cnt, low, AtomicAdd());
}

__global__ void __launch_bounds__(256) dvp_pairs_scores(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ low, int N, uint32_t* __restrict__ score) {
	const uint32_t at = blockIdx.x * 256u + threadIdx.x;
	if (at >= (uint32_t)N * (uint32_t)N) return;
	score[at] = score_at(cnt, low, N, (int)(at / (uint32_t)N), (int)(at % (uint32_t)N));
}

__global__ void __launch_bounds__(256) dvp_pairs_convert(const uint8_t* __restrict__ bgr, int w, int h, size_t pitch, int pad_w, int pad_h, int out_w, int out_h, uint8_t* __restrict__ out) {
	const int k = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
	if (k >= 3 * out_w || y >= out_h) return;
	out[(size_t)y * 3 * out_w + k] = converted_byte(bgr, w, h, pitch, pad_w, pad_h, out_w, out_h, k, y);
}

}   // namespace dvppairs

static thread_local dvpmem::CallError t_pairs_error;
static int pairs_fail(const char* who, const std::string& what) { return t_pairs_error.fail(who, what); }

extern "C" const char* dvp_pairs_last_error(void) { return t_pairs_error.c_str(); }

extern "C" int dvp_view_scores(int device, int num_images, const long long* obs_offsets, const long long* obs_point_ids, const double* centres, long long num_points,
                               const long long* point_ids, const double* xyz, uint32_t* score_out) {
	using namespace dvppairs;
	const char* who = "dvp_view_scores";
	t_pairs_error.clear();
	if (!obs_offsets || !centres || !score_out) return pairs_fail(who, "obs_offsets, centres and score_out are required");
	if (num_images >= 1 && num_images <= kMaxImages && obs_offsets[num_images] > 0 && !obs_point_ids) return pairs_fail(who, "obs_point_ids is required");
	if (num_points > 0 && (!point_ids || !xyz)) return pairs_fail(who, "point_ids and xyz are required");
	TrackArrays arrays;
	const std::string what = build_tracks(num_images, obs_offsets, obs_point_ids, num_points, point_ids, &arrays);
	if (!what.empty()) return pairs_fail(who, what);
	const size_t N = (size_t)num_images, P = (size_t)num_points, E = arrays.image.size();
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return pairs_fail(who, "hipSetDevice failed"); }
	dvpmem::DevBlock pool;
	dvpmem::StreamScope st;
	if (st.open()) return pairs_fail(who, "hipStreamCreate failed");
	dvpmem::Carve c;
	const size_t o_off = c.take((P + 1) * 4), o_point = c.take(E * 4), o_image = c.take(E * 4), o_mult = c.take(E * 4), o_xyz = c.take(P * 24), o_centres = c.take(N * 24),
	             o_cnt = c.take(N * N * 4), o_low = c.take(N * N * 4), o_score = c.take(N * N * 4);
	if (pool.reserve(c.total)) return pairs_fail(who, "out of device memory");
	uint8_t* b = pool.as<uint8_t>();
	auto up = [&](size_t at, const void* src, size_t bytes) { return bytes == 0 || hipMemcpyAsync(b + at, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess; };
	if (!up(o_off, arrays.off.data(), (P + 1) * 4) || !up(o_point, arrays.point.data(), E * 4) || !up(o_image, arrays.image.data(), E * 4) || !up(o_mult, arrays.mult.data(), E * 4) ||
	    !up(o_xyz, xyz, P * 24) || !up(o_centres, centres, N * 24) || hipMemsetAsync(b + o_cnt, 0, o_score - o_cnt, st) != hipSuccess) {   // (cnt and low lie side by side)
		(void)hipGetLastError();
		return pairs_fail(who, "upload failed");
	}
	const Tracks t{ (const uint32_t*)(b + o_off), (const uint32_t*)(b + o_point), (const uint32_t*)(b + o_image), (const uint32_t*)(b + o_mult), (const double*)(b + o_xyz), (const double*)(b + o_centres) };
	if (E) hipLaunchKernelGGL(dvp_pairs_count, dim3((unsigned)((E + 3) / 4)), dim3(256), 0, st, t, (uint32_t)E, num_images, (uint32_t*)(b + o_cnt), (uint32_t*)(b + o_low));
	hipLaunchKernelGGL(dvp_pairs_scores, dim3((unsigned)((N * N + 255) / 256)), dim3(256), 0, st, (const uint32_t*)(b + o_cnt), (const uint32_t*)(b + o_low), num_images, (uint32_t*)(b + o_score));
	if (hipGetLastError() != hipSuccess) return pairs_fail(who, "launch failed");
	if (hipMemcpyAsync(score_out, b + o_score, N * N * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
		(void)hipGetLastError();
		return pairs_fail(who, "the scores could not be made or fetched");
	}
	return 0;
}

extern "C" int dvp_convert_image(int device, const uint8_t* bgr, int w, int h, long long pitch, int pad_w, int pad_h, int out_w, int out_h, uint8_t* out) {
	using namespace dvppairs;
	const char* who = "dvp_convert_image";
	t_pairs_error.clear();
	const std::string what = check_convert(bgr, w, h, pitch, pad_w, pad_h, out_w, out_h, out);
	if (!what.empty()) return pairs_fail(who, what);
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return pairs_fail(who, "hipSetDevice failed"); }
	dvpmem::DevBlock pool;
	dvpmem::StreamScope st;
	if (st.open()) return pairs_fail(who, "hipStreamCreate failed");
	const size_t row = 3 * (size_t)w, out_row = 3 * (size_t)out_w;
	dvpmem::Carve c;
	const size_t o_in = c.take(row * h), o_out = c.take(out_row * out_h);
	if (pool.reserve(c.total)) return pairs_fail(who, "out of device memory");
	uint8_t* b = pool.as<uint8_t>();
	if (hipMemcpy2DAsync(b + o_in, row, bgr, (size_t)pitch, row, (size_t)h, hipMemcpyHostToDevice, st) != hipSuccess) { (void)hipGetLastError(); return pairs_fail(who, "upload failed"); }
	hipLaunchKernelGGL(dvp_pairs_convert, dim3((unsigned)((out_row + 255) / 256), (unsigned)out_h), dim3(256), 0, st, b + o_in, w, h, row, pad_w, pad_h, out_w, out_h, b + o_out);
	if (hipGetLastError() != hipSuccess) return pairs_fail(who, "launch failed");
	if (hipMemcpyAsync(out, b + o_out, out_row * out_h, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
		(void)hipGetLastError();
		return pairs_fail(who, "the image could not be made or fetched");
	}
	return 0;
}
