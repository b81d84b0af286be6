// Host build of the device edge prior's steps (dvp-mvs_amd/csrc/dvp_edges.hpp), one pixel after the other (TEST
// INFRASTRUCTURE): lets the CPU tests hold the kernels' arithmetic against the host mirror's EdgeSegment and the numpy Canny
// without a GPU.  Same stages, same order, same buffers as dvp_edges.hip.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../dvp-mvs_amd/csrc/dvp_edges.hpp"

using namespace dvpedge;

namespace {
struct HostMem {   // one thread: plain memory operations
	unsigned load(const unsigned* p) const { return *p; }
	unsigned min(unsigned* p, unsigned v) const { const unsigned o = *p; if (v < o) *p = v; return o; }
};
struct BytePx {
	const uint8_t* p; long long pitch;
	int operator()(int y, int x) const { return p[(long long)y * pitch + x]; }
};
struct RawPx {
	const uint8_t* raw; int W;
	bool operator()(int y, int x) const { return raw[(size_t)y * W + x] != 0; }
};
void hysteresis(const uint8_t* map3, int W, int H, uint8_t* raw) {
	const size_t L = (size_t)W * H;
	std::vector<unsigned> parent(L);
	std::vector<uint8_t> mark(L, 0);
	for (size_t i = 0; i < L; ++i) parent[i] = (unsigned)i;
	HostMem mem;
	for (int y = 0; y < H; ++y)
		for (int x = 0; x < W; ++x) merge_pixel(mem, map3, parent.data(), x, y, W, H);
	for (size_t i = 0; i < L; ++i) {
		if (map3[i] == MAP_NONE) continue;
		const unsigned r = uf_find(mem, parent.data(), (unsigned)i);
		mem.min(&parent[i], r);
		if (map3[i] == MAP_STRONG) mark[r] = 1;
	}
	for (size_t i = 0; i < L; ++i) raw[i] = (map3[i] == MAP_STRONG || (map3[i] == MAP_CANDIDATE && mark[parent[i]])) ? 255 : 0;
}
}   // namespace

extern "C" void dvp_edge_thresholds_host(int median, int* low, int* high) { thresholds_of_median(median, low, high); }

extern "C" int dvp_edge_median_host(const uint8_t* grey, int W, int H, long long pitch) {
	unsigned hist[256] = { 0 };
	for (int y = 0; y < H; ++y)
		for (int x = 0; x < W; ++x) hist[grey[(long long)y * pitch + x]]++;
	return median_of(hist, W * H);
}

extern "C" void dvp_grey_bytes_host(const float* texels, long long n, uint8_t* out) {
	for (long long i = 0; i < n; ++i) out[i] = grey_byte(texels[i]);
}

extern "C" int dvp_edge_hysteresis_host(const uint8_t* map3, int W, int H, uint8_t* edge_out) {
	if (!map3 || !edge_out || W < 1 || H < 1) return 1;
	hysteresis(map3, W, H, edge_out);
	return 0;
}

extern "C" int dvp_canny_edge_map_host(const uint8_t* grey, int W, int H, long long pitch, uint8_t* edge_out) {
	if (!grey || !edge_out || W < 3 || H < 3 || pitch < W) return 1;
	int low, high;
	thresholds_of_median(dvp_edge_median_host(grey, W, H, pitch), &low, &high);
	const size_t L = (size_t)W * H;
	std::vector<uint8_t> map3(L), raw(L);
	const BytePx px{ grey, pitch };
	for (int y = 0; y < H; ++y)
		for (int x = 0; x < W; ++x) map3[(size_t)y * W + x] = map3_at(px, x, y, W, H, low, high);
	hysteresis(map3.data(), W, H, raw.data());
	const RawPx rp{ raw.data(), W };
	for (int y = 0; y < H; ++y)
		for (int x = 0; x < W; ++x) edge_out[(size_t)y * W + x] = fixed_at(rp, x, y, W, H);
	return 0;
}
