// dvp_edges.hip — the depth-edge prior on the device: EdgeSegment(scale, image, 0, true) (APD.cpp:404-466), the median-adaptive
// Canny the driver's helper threads ran per view (host/edges.cpp).  The arithmetic lives in dvp_edges.hpp; this file maps it
// onto the GPU with a fixed sequence of launches and no host wait:
//   dvp_edge_grey_hist     grey bytes (from a float plane) + 256-bin histogram: per-wave counts in LDS, summed per work-group,
//                          one global atomic per non-empty bin and group
//   dvp_edge_thresholds    one lane: median -> (low, high), kept in device memory
//   dvp_edge_suppress      Sobel + magnitude + sector suppression from a 36 x 12 LDS tile of bytes -> three-state map
//                          (the magnitude is recomputed for the two neighbours the sector names; no 4-byte plane)
//   dvp_edge_uf_init / _merge / _flatten / _resolve
//                          hysteresis as label equivalence: every non-empty pixel unites with its forward neighbours
//                          (E, SW, S, SE) by atomicMin on roots, retried until it holds; links are flattened; strong pixels
//                          mark their root; candidates read their root's mark.  Four launches whatever the content.
//   dvp_edge_fixups        the frame fix-ups with their sequential meaning, written to one or two maps
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/dvp_mvs.h"
#include "dvp_edges_run.h"

namespace dvpedge {

constexpr int kHistBlocks = 1024;   // at most this many work-groups: <= 256 global atomics each

// src != nullptr: grey[i] = grey_byte(src[(y * pitch + x) * step]) first; then the histogram of grey
__global__ void __launch_bounds__(256) dvp_edge_grey_hist(const float* __restrict__ src, long long pitch, int step, uint8_t* __restrict__ grey, int W, size_t L,
                                                          unsigned* __restrict__ hist) {
	__shared__ unsigned h[4][256];
	const int tid = threadIdx.x;
	for (int k = 0; k < 4; ++k) h[k][tid] = 0;
	__syncthreads();
	unsigned* mine = h[tid >> 6];
	for (size_t i = (size_t)blockIdx.x * 256 + tid; i < L; i += (size_t)gridDim.x * 256) {
		uint8_t v;
		if (src) {
			const size_t y = i / (size_t)W, x = i - y * (size_t)W;
			v = grey_byte(src[(y * (size_t)pitch + x) * (size_t)step]);
			grey[i] = v;
		} else v = grey[i];
		atomicAdd(&mine[v], 1u);
	}
	__syncthreads();
	const unsigned n = h[0][tid] + h[1][tid] + h[2][tid] + h[3][tid];
	if (n) atomicAdd(&hist[tid], n);
}

__global__ void dvp_edge_thresholds(unsigned* __restrict__ hist, int pixels) {
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	int low, high;
	thresholds_of_median(median_of(hist, pixels), &low, &high);
	hist[256] = (unsigned)low;
	hist[257] = (unsigned)high;
}

constexpr int kTileW = 32, kTileH = 8, kHalo = 2;
struct TilePx {
	const uint8_t* t;   // [kTileH + 2 * kHalo][kTileW + 2 * kHalo]
	int x0, y0;         // image coordinates of t[0][0]
	__device__ int operator()(int y, int x) const { return t[(y - y0) * (kTileW + 2 * kHalo) + (x - x0)]; }
};
__global__ void __launch_bounds__(kTileW * kTileH) dvp_edge_suppress(const uint8_t* __restrict__ grey, int W, int H, const unsigned* __restrict__ hist, uint8_t* __restrict__ map3) {
	constexpr int TW = kTileW + 2 * kHalo, TH = kTileH + 2 * kHalo;
	__shared__ uint8_t tile[TH * TW];
	const int tx0 = blockIdx.x * kTileW - kHalo, ty0 = blockIdx.y * kTileH - kHalo;
	const int tid = threadIdx.y * kTileW + threadIdx.x;
	for (int k = tid; k < TH * TW; k += kTileW * kTileH) {
		const int gx = tx0 + k % TW, gy = ty0 + k / TW;
		// positions outside the image are never read: Sobel clamps its coordinates into the image first
		tile[k] = (gx >= 0 && gy >= 0 && gx < W && gy < H) ? grey[(size_t)gy * W + gx] : (uint8_t)0;
	}
	__syncthreads();
	const int x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
	if (x >= W || y >= H) return;
	const TilePx px{ tile, tx0, ty0 };
	map3[(size_t)y * W + x] = map3_at(px, x, y, W, H, (int)hist[256], (int)hist[257]);
}

__global__ void __launch_bounds__(256) dvp_edge_uf_init(unsigned* __restrict__ parent, uint8_t* __restrict__ mark, size_t L) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= L) return;
	parent[i] = (unsigned)i;
	mark[i] = 0;
}
__global__ void __launch_bounds__(256) dvp_edge_uf_merge(const uint8_t* __restrict__ map3, unsigned* parent, int W, int H) {
	const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
	if (x >= W || y >= H) return;
	DevMem mem;
	merge_pixel(mem, map3, parent, x, y, W, H);
}
// no unions run any more: uf_find returns the set's final root
__global__ void __launch_bounds__(256) dvp_edge_uf_flatten(const uint8_t* __restrict__ map3, unsigned* parent, uint8_t* mark, size_t L) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= L) return;
	const uint8_t m = map3[i];
	if (m == MAP_NONE) return;
	DevMem mem;
	const unsigned r = uf_find(mem, parent, (unsigned)i);
	mem.min(parent + i, r);
	if (m == MAP_STRONG) mark[r] = 1;   // (every writer stores the same byte)
}
__global__ void __launch_bounds__(256) dvp_edge_uf_resolve(const uint8_t* __restrict__ map3, const unsigned* __restrict__ parent, const uint8_t* __restrict__ mark, uint8_t* __restrict__ raw, size_t L) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= L) return;
	const uint8_t m = map3[i];
	raw[i] = (m == MAP_STRONG || (m == MAP_CANDIDATE && mark[parent[i]])) ? (uint8_t)255 : (uint8_t)0;
}

struct RawPx {
	const uint8_t* raw;
	int W;
	__device__ bool operator()(int y, int x) const { return raw[(size_t)y * W + x] != 0; }
};
__global__ void __launch_bounds__(256) dvp_edge_fixups(const uint8_t* __restrict__ raw, int W, int H, uint8_t* __restrict__ out, uint8_t* __restrict__ out2) {
	const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
	if (x >= W || y >= H) return;
	const size_t i = (size_t)y * W + x;
	const bool frame = x == 0 || y == 0 || x == W - 1 || y == H - 1;
	const uint8_t v = frame ? fixed_at(RawPx{ raw, W }, x, y, W, H) : raw[i];   // W, H >= 3: columns 1, W - 2 and rows 1, H - 2 exist
	out[i] = v;
	if (out2) out2[i] = v;
}

int scratch_reserve(Scratch& s, size_t pixels) {
	const size_t n = pixels ? pixels : 1;
	dvpmem::Carve c;
	const size_t o_grey = c.take(n), o_map3 = c.take(n), o_mark = c.take(n), o_parent = c.take(n * 4), o_hist = c.take(258 * 4);
	if (s.block.reserve(c.total)) { scratch_free(s); return 1; }
	uint8_t* b = s.block.as<uint8_t>();
	s.grey = b + o_grey; s.map3 = b + o_map3; s.mark = b + o_mark; s.parent = (unsigned*)(b + o_parent); s.hist = (unsigned*)(b + o_hist);
	return 0;
}
void scratch_free(Scratch& s) {
	s.block.release();
	s.grey = s.map3 = s.mark = nullptr;
	s.parent = s.hist = nullptr;
}

static unsigned blocks1d(size_t L) { return (unsigned)((L + 255) / 256); }
static dim3 blocks2d(int W, int H) { return dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)); }

static int grey_hist(hipStream_t stream, Scratch& s, const float* src, long long pitch, int step, int W, int H) {
	const size_t L = (size_t)W * H;
	if (hipMemsetAsync(s.hist, 0, 258 * 4, stream) != hipSuccess) return 1;
	const size_t want = (L + 256 * 16 - 1) / (256 * 16);
	const unsigned grid = (unsigned)(want < 1 ? 1 : (want > (size_t)kHistBlocks ? (size_t)kHistBlocks : want));
	hipLaunchKernelGGL(dvp_edge_grey_hist, dim3(grid), dim3(256), 0, stream, src, pitch, step, s.grey, W, L, s.hist);
	return hipGetLastError() != hipSuccess;
}
int launch_grey_from_float(hipStream_t stream, Scratch& s, const float* src, long long pitch, int step, int W, int H) {
	return grey_hist(stream, s, src, pitch, step, W, H);
}
int launch_suppress(hipStream_t stream, Scratch& s, int W, int H, bool have_hist) {
	if (!have_hist && grey_hist(stream, s, nullptr, 0, 0, W, H)) return 1;
	hipLaunchKernelGGL(dvp_edge_thresholds, dim3(1), dim3(64), 0, stream, s.hist, W * H);
	hipLaunchKernelGGL(dvp_edge_suppress, dim3((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH)), dim3(kTileW, kTileH), 0, stream,
	                   s.grey, W, H, s.hist, s.map3);
	return hipGetLastError() != hipSuccess;
}
int launch_hysteresis(hipStream_t stream, Scratch& s, int W, int H) {
	const size_t L = (size_t)W * H;
	hipLaunchKernelGGL(dvp_edge_uf_init, dim3(blocks1d(L)), dim3(256), 0, stream, s.parent, s.mark, L);
	hipLaunchKernelGGL(dvp_edge_uf_merge, blocks2d(W, H), dim3(64, 4), 0, stream, s.map3, s.parent, W, H);
	hipLaunchKernelGGL(dvp_edge_uf_flatten, dim3(blocks1d(L)), dim3(256), 0, stream, s.map3, s.parent, s.mark, L);
	hipLaunchKernelGGL(dvp_edge_uf_resolve, dim3(blocks1d(L)), dim3(256), 0, stream, s.map3, s.parent, s.mark, s.grey, L);
	return hipGetLastError() != hipSuccess;
}
int launch_fixups(hipStream_t stream, Scratch& s, int W, int H, uint8_t* out, uint8_t* out2) {
	hipLaunchKernelGGL(dvp_edge_fixups, blocks2d(W, H), dim3(64, 4), 0, stream, s.grey, W, H, out, out2);
	return hipGetLastError() != hipSuccess;
}

}   // namespace dvpedge

// ---- the two context-free calls: host in, host out ---------------------------------------------------------------------------
static thread_local dvpmem::CallError t_edge_error;

extern "C" const char* dvp_edge_last_error(void) { return t_edge_error.c_str(); }

// src: `pitch` bytes per row; full = stages 2-6 on grey bytes, else stage 5 on a three-state map
static int edge_call(const char* who, int device, const uint8_t* src, int W, int H, long long pitch, uint8_t* dst, bool full) {
	t_edge_error.clear();
	auto fail = [who](const char* what) { return t_edge_error.fail(who, what); };
	if (!src || !dst) return fail("input and output pointers are required");
	if (full && (W < 3 || H < 3)) return fail("width and height must be at least 3 (the frame fix-ups read columns 1, W - 2 and rows 1, H - 2)");
	if (W < 1 || H < 1 || (long long)W * H > 0x7fffffffLL || pitch < W) return fail("bad image geometry");
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return fail("hipSetDevice failed"); }
	dvpedge::Scratch s;
	dvpmem::DevBlock d_out;
	dvpmem::StreamScope st;
	if (st.open()) return fail("hipStreamCreate failed");
	const size_t L = (size_t)W * H;
	if (dvpedge::scratch_reserve(s, L)) return fail("out of device memory");
	if (hipMemcpy2DAsync(full ? s.grey : s.map3, (size_t)W, src, (size_t)pitch, (size_t)W, (size_t)H, hipMemcpyHostToDevice, st) != hipSuccess) return fail("upload failed");
	if (full && dvpedge::launch_suppress(st, s, W, H, false)) return fail("launch failed");
	if (dvpedge::launch_hysteresis(st, s, W, H)) return fail("launch failed");
	const uint8_t* result = s.grey;
	if (full) {
		if (d_out.reserve(L)) return fail("out of device memory");
		if (dvpedge::launch_fixups(st, s, W, H, d_out.as<uint8_t>(), nullptr)) return fail("launch failed");
		result = d_out.as<uint8_t>();
	}
	if (hipMemcpyAsync(dst, result, L, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail("download failed");
	return 0;
}

extern "C" int dvp_canny_edge_map(int device, const uint8_t* grey, int width, int height, long long pitch_bytes, uint8_t* edge_out) {
	return edge_call("dvp_canny_edge_map", device, grey, width, height, pitch_bytes, edge_out, true);
}

extern "C" int dvp_edge_hysteresis(int device, const uint8_t* map3, int width, int height, uint8_t* edge_out) {
	return edge_call("dvp_edge_hysteresis", device, map3, width, height, (long long)width, edge_out, false);
}
