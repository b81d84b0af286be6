// dvp_undistort.hip — the device half of `apd --convert-from ... --undistort on`: one launch per picture resamples it into the pinhole
// camera of its COLMAP camera.  The arithmetic, the argument checks and the serial form live in dvp_undistort.hpp.
//   dvp_undistort_rows   a wave is 64 x-adjacent output pixels of one row, a work-group four such waves.  The camera travels by value
//                        (104 bytes of kernel arguments: the model switch is uniform).  Each lane forms its binary64 source
//                        coordinates - about 100 operations, three square roots and four divisions of them in the fisheye models'
//                        atan - and gathers 4 taps x 3 channels as bytes.  No coordinate map is stored: reading 8 bytes per pixel
//                        back would cost more than computing them again.
//   The stores.  A lane per pixel leaves 3 bytes.  The work-group's 768 bytes go through LDS and leave as 192 32-bit words, lane k
//   storing word k: a wave's store instruction covers 256 contiguous bytes.  The other form - a lane making four pixels and storing
//   their 12 bytes as three words, a wave 256 pixels - was built and measured too and is not kept: a 6208 x 4128 THIN_PRISM_FISHEYE
//   picture takes 0.29 ms this way and 0.44 ms that way on an MI355X (profiles/convert.txt).  Both need rows that start on a word:
//   the device picture has a pitch of 3 * w rounded up to 4 bytes and goes back to the host's dense rows with a 2-D copy (a plain
//   one when 3 * w is a multiple of 4).
// Bounds: a word is stored when its first byte lies in the row (below 3 * w), so it ends inside the row's pitch; the gathers clamp
// (undistorted_pixel reads no row or column that is outside).  Byte offsets are formed in size_t; gridDim.y = h <= 65535.
// Device memory: one DevBlock per call, carved; the stream of a call is a StreamScope.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/dvp_mvs.h"
#include "dvp_devmem.hpp"
#include "dvp_undistort.hpp"

namespace dvpund {

constexpr int kPixelsPerGroup = 256;
__global__ void __launch_bounds__(256) dvp_undistort_rows(const Camera cam, const uint8_t* __restrict__ bgr, int w, int h, size_t pitch, uint8_t* __restrict__ out, size_t out_pitch) {
	__shared__ uint32_t words[192];
	uint8_t* bytes = reinterpret_cast<uint8_t*>(words);
	const int x0 = blockIdx.x * 256, x = x0 + (int)threadIdx.x, y = blockIdx.y;
	uint8_t px[3] = { 0, 0, 0 };
	if (x < w) undistorted_pixel(cam, bgr, w, h, pitch, x, y, px);
	bytes[3 * threadIdx.x] = px[0];
	bytes[3 * threadIdx.x + 1] = px[1];
	bytes[3 * threadIdx.x + 2] = px[2];
	__syncthreads();
	const size_t at = 3 * (size_t)x0 + 4 * (size_t)threadIdx.x;   // byte offset in the row, a multiple of 4
	if (threadIdx.x < 192 && at < 3 * (size_t)w) *reinterpret_cast<uint32_t*>(out + (size_t)y * out_pitch + at) = words[threadIdx.x];
}

}   // namespace dvpund

static thread_local dvpmem::CallError t_undistort_error;
static int undistort_fail(const std::string& what) { return t_undistort_error.fail("dvp_undistort_image", what); }

extern "C" const char* dvp_undistort_last_error(void) { return t_undistort_error.c_str(); }

extern "C" int dvp_undistort_image(int device, const uint8_t* bgr, int w, int h, long long pitch, int model, const double* params, int num_params, uint8_t* out) {
	using namespace dvpund;
	t_undistort_error.clear();
	const std::string what = check_undistort(bgr, w, h, pitch, model, params, num_params, out);
	if (!what.empty()) return undistort_fail(what);
	const Camera cam = make_camera(model, params);
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return undistort_fail("hipSetDevice failed"); }
	dvpmem::DevBlock pool;
	dvpmem::StreamScope st;
	if (st.open()) return undistort_fail("hipStreamCreate failed");
	const size_t row = 3 * (size_t)w, out_pitch = (row + 3) & ~(size_t)3;
	dvpmem::Carve c;
	const size_t o_in = c.take(row * h), o_out = c.take(out_pitch * h);
	if (pool.reserve(c.total)) return undistort_fail("out of device memory");
	uint8_t* b = pool.as<uint8_t>();
	if (hipMemcpy2DAsync(b + o_in, row, bgr, (size_t)pitch, row, (size_t)h, hipMemcpyHostToDevice, st) != hipSuccess) { (void)hipGetLastError(); return undistort_fail("upload failed"); }
	hipLaunchKernelGGL(dvp_undistort_rows, dim3((unsigned)((w + kPixelsPerGroup - 1) / kPixelsPerGroup), (unsigned)h), dim3(256), 0, st, cam, b + o_in, w, h, row, b + o_out, out_pitch);
	if (hipGetLastError() != hipSuccess) return undistort_fail("launch failed");
	const hipError_t back = out_pitch == row ? hipMemcpyAsync(out, b + o_out, row * h, hipMemcpyDeviceToHost, st)
	                                         : hipMemcpy2DAsync(out, row, b + o_out, out_pitch, row, (size_t)h, hipMemcpyDeviceToHost, st);
	if (back != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
		(void)hipGetLastError();
		return undistort_fail("the image could not be made or fetched");
	}
	return 0;
}
