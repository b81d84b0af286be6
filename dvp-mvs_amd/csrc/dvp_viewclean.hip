// dvp_viewclean.hip — ProcessProblem's visibility-mask clean-up (main.cpp:311-363) on the device: per source view, every
// 4-connected region of pixels that do NOT select the view and is smaller than min_region pixels is switched to "selected".  The
// arithmetic lives in dvp_viewclean.hpp; this file maps it onto the GPU with four launches whatever the words hold, and no host wait:
//   dvp_vc_tiles     a work-group of four waves owns a 64 x 16 tile and labels it in LDS, plane after plane from the words it read
//                    once: a row's clear pixels are one __ballot, its runs come from bit arithmetic on that mask (no atomics), the
//                    runs of adjacent rows are united by LDS atomicMin on tile-local labels, a run adds its length to its local
//                    root's LDS counter.  A pixel's parent word becomes the global index of its local root, the root's size word
//                    the count.  The pixels that do not select a view are often most of the image, in components of millions of
//                    pixels: this step keeps their unions and their counts out of global memory
//   dvp_vc_seams     the pixels on a tile's last column / last row unite with their E / S neighbour: atomicMin on roots, retried
//                    until it holds, every parent word read by a device-scope atomic load (uf_union with DevMem, as the edge
//                    prior's hysteresis)
//   dvp_vc_rollup    a local root that is not its component's root adds its count to the root's: one atomic per tile and component
//   dvp_vc_resolve   one lane per word: every clear bit follows its parent words to the root, reads the size and is set when the
//                    region is too small; the bits >= num_src are dropped
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/dvp_mvs.h"
#include "dvp_edges_run.h"
#include "dvp_viewclean_run.h"

namespace dvpvc {

// the tile's words in LDS: other waves of the work-group unite and count on them between two barriers
struct LdsMem {
	__device__ unsigned load(const unsigned* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
	__device__ unsigned min(unsigned* p, unsigned v) const { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
	__device__ unsigned add(unsigned* p, unsigned v) const { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
// the global words: dvp_edges' device-scope loads and atomicMin, plus the size roll-up's addition
struct AgentMem : dvpedge::DevMem {
	__device__ unsigned add(unsigned* p, unsigned v) const { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

constexpr int kWaves = 4, kRowsPerWave = TILE_H / kWaves;

__global__ void __launch_bounds__(TILE_W * kWaves) dvp_vc_tiles(const uint32_t* __restrict__ views, int W, int H, int num_src, unsigned* __restrict__ parent,
                                                               unsigned* __restrict__ size, size_t L) {
	__shared__ unsigned lab[TILE_PIXELS], cnt[TILE_PIXELS];
	__shared__ uint64_t rows[TILE_H];
	const int lane = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * kRowsPerWave;
	const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H, x = x0 + lane;
	uint32_t word[kRowsPerWave];
	for (int k = 0; k < kRowsPerWave; ++k) {
		const int y = y0 + r0 + k;
		word[k] = (x < W && y < H) ? views[(size_t)y * W + x] : 0xffffffffu;   // outside the image: never clear
	}
	LdsMem mem;
	for (int b = 0; b < num_src; ++b) {
		for (int k = 0; k < kRowsPerWave; ++k) tile_init(lab, cnt, rows, r0 + k, lane, (uint64_t)__ballot(!((word[k] >> b) & 1u)));
		__syncthreads();
		for (int k = 0; k < kRowsPerWave; ++k) tile_union_up(mem, lab, rows, r0 + k, lane);
		__syncthreads();
		for (int k = 0; k < kRowsPerWave; ++k) tile_count(mem, lab, cnt, rows, r0 + k, lane);
		__syncthreads();
		for (int k = 0; k < kRowsPerWave; ++k) tile_store(mem, lab, cnt, rows, r0 + k, lane, x0, y0, W, H, parent + (size_t)b * L, size + (size_t)b * L);
		__syncthreads();   // the next plane's tile_init writes the same words
	}
}

__global__ void __launch_bounds__(256) dvp_vc_seams(const uint32_t* __restrict__ views, int W, int H, unsigned* parent, size_t L, size_t items) {
	const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= items) return;
	AgentMem mem;
	seam_item(mem, views, (int)blockIdx.y, parent + (size_t)blockIdx.y * L, t, W, H);
}

__global__ void __launch_bounds__(256) dvp_vc_rollup(unsigned* parent, unsigned* size, size_t L) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= L) return;
	AgentMem mem;
	rollup_pixel(mem, parent + (size_t)blockIdx.y * L, size + (size_t)blockIdx.y * L, i);
}

// (out may be views: a lane reads its own word only, before it writes it)
__global__ void __launch_bounds__(256) dvp_vc_resolve(const uint32_t* views, int num_src, int min_region, const unsigned* __restrict__ parent, const unsigned* __restrict__ size,
                                                      size_t L, uint32_t* out) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= L) return;
	out[i] = resolve_word(views[i], num_src, min_region, parent, size, L, i);
}

int scratch_reserve(Scratch& s, size_t pixels, int planes) { return s.block.reserve(pixels * (size_t)(planes > 0 ? planes : 0) * 2 * 4); }
void scratch_free(Scratch& s) { s.block.release(); }

// steps 1-3: after them parent leads every clear pixel to its component's root, whose size word holds the component's pixels
int launch_components(hipStream_t stream, Scratch& s, const uint32_t* views, int W, int H, int num_src) {
	const size_t L = (size_t)W * H;
	unsigned* parent = s.words();
	unsigned* size = parent + (size_t)num_src * L;
	const unsigned per_pixel = (unsigned)((L + 255) / 256);
	if (num_src > 0) {
		hipLaunchKernelGGL(dvp_vc_tiles, dim3((unsigned)((W + TILE_W - 1) / TILE_W), (unsigned)((H + TILE_H - 1) / TILE_H)), dim3(TILE_W * kWaves), 0, stream, views, W, H, num_src,
		                   parent, size, L);
		const size_t items = seam_items(W, H);   // (none in an image of one tile: the launch stays, with one idle work-group per plane)
		hipLaunchKernelGGL(dvp_vc_seams, dim3((unsigned)((items + 255) / 256 > 0 ? (items + 255) / 256 : 1), (unsigned)num_src), dim3(256), 0, stream, views, W, H, parent, L, items);
		hipLaunchKernelGGL(dvp_vc_rollup, dim3(per_pixel, (unsigned)num_src), dim3(256), 0, stream, parent, size, L);
	}
	return hipGetLastError() != hipSuccess;
}

int launch_clean(hipStream_t stream, Scratch& s, const uint32_t* views, int W, int H, int num_src, int min_region, uint32_t* out) {
	const size_t L = (size_t)W * H;
	if (launch_components(stream, s, views, W, H, num_src)) return 1;
	hipLaunchKernelGGL(dvp_vc_resolve, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, stream, views, num_src, min_region, s.words(), s.words() + (size_t)num_src * L, L, out);
	return hipGetLastError() != hipSuccess;
}

}   // namespace dvpvc

// ---- the context-free call: host in, host out ---------------------------------------------------------------------------------
static thread_local dvpmem::CallError t_vc_error;

extern "C" const char* dvp_viewclean_last_error(void) { return t_vc_error.c_str(); }

extern "C" int dvp_clean_selected_views(int device, const uint32_t* views, int W, int H, int num_src, int min_region, uint32_t* out) {
	t_vc_error.clear();
	auto fail = [](const char* what) { return t_vc_error.fail("dvp_clean_selected_views", what); };
	if (!views || !out) return fail("input and output pointers are required");
	if (num_src < 0 || num_src > 32) return fail("num_src must be 0 ... 32 (one bit of a word per source view)");
	if (W < 1 || H < 1 || (long long)W * H > 0x7fffffffLL) return fail("bad image geometry");
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return fail("hipSetDevice failed"); }
	dvpvc::Scratch s;
	dvpmem::DevBlock d_views;
	dvpmem::StreamScope st;
	if (st.open()) return fail("hipStreamCreate failed");
	const size_t L = (size_t)W * H;
	if (dvpvc::scratch_reserve(s, L, num_src) || d_views.reserve(L * 4)) return fail("out of device memory");
	uint32_t* words = d_views.as<uint32_t>();
	if (hipMemcpyAsync(words, views, L * 4, hipMemcpyHostToDevice, st) != hipSuccess) return fail("upload failed");
	if (dvpvc::launch_clean(st, s, words, W, H, num_src, min_region, words)) return fail("launch failed");
	if (hipMemcpyAsync(out, words, L * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail("download failed");
	return 0;
}
