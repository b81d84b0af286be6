// Host build of the device view clean-up's steps (dvp-mvs_amd/csrc/dvp_viewclean.hpp), one tile, one lane after the other (TEST
// INFRASTRUCTURE): lets the CPU tests hold the kernels' arithmetic against the host mirror's clean-up and scipy's components
// without a GPU.  Same steps, same order, same words as dvp_viewclean.hip; a row's mask is gathered lane by lane where the
// device has __ballot.  The second export is the host mirror itself: host/cc.cpp's Connect + the fill rule of the driver's
// background job (host/main.cpp, ProcessProblem) on a word map, with the job's team of up to eight threads.
#include <stdint.h>
#include <vector>

#include "../../dvp-mvs_amd/csrc/dvp_viewclean.hpp"
#include "../../dvp-mvs_amd/host/APD.h"

using namespace dvpvc;

namespace {
struct HostMem {   // one thread: plain memory operations
	unsigned load(const unsigned* p) const { return *p; }
	unsigned min(unsigned* p, unsigned v) const { const unsigned o = *p; if (v < o) *p = v; return o; }
	unsigned add(unsigned* p, unsigned v) const { const unsigned o = *p; *p = o + v; return o; }
};
}   // namespace

extern "C" int dvp_viewclean_tile_w(void) { return TILE_W; }
extern "C" int dvp_viewclean_tile_h(void) { return TILE_H; }

extern "C" int dvp_clean_selected_views_serial(const uint32_t* views, int W, int H, int num_src, int min_region, uint32_t* out) {
	if (!views || !out || W < 1 || H < 1 || num_src < 0 || num_src > 32) return 1;
	const size_t L = (size_t)W * H;
	std::vector<unsigned> parent(L * (size_t)num_src), size(L * (size_t)num_src);
	HostMem mem;
	unsigned lab[TILE_PIXELS], cnt[TILE_PIXELS];
	uint64_t rows[TILE_H];
	for (int b = 0; b < num_src; ++b) {
		unsigned* par = parent.data() + (size_t)b * L;
		unsigned* siz = size.data() + (size_t)b * L;
		for (int y0 = 0; y0 < H; y0 += TILE_H)
			for (int x0 = 0; x0 < W; x0 += TILE_W) {
				for (int r = 0; r < TILE_H; ++r) {
					uint64_t clear = 0;
					for (int lane = 0; lane < TILE_W; ++lane) {
						const int x = x0 + lane, y = y0 + r;
						const uint32_t word = (x < W && y < H) ? views[(size_t)y * W + x] : 0xffffffffu;
						if (!((word >> b) & 1u)) clear |= (uint64_t)1 << lane;
					}
					for (int lane = 0; lane < TILE_W; ++lane) tile_init(lab, cnt, rows, r, lane, clear);
				}
				for (int r = 0; r < TILE_H; ++r)
					for (int lane = 0; lane < TILE_W; ++lane) tile_union_up(mem, lab, rows, r, lane);
				for (int r = 0; r < TILE_H; ++r)
					for (int lane = 0; lane < TILE_W; ++lane) tile_count(mem, lab, cnt, rows, r, lane);
				for (int r = 0; r < TILE_H; ++r)
					for (int lane = 0; lane < TILE_W; ++lane) tile_store(mem, lab, cnt, rows, r, lane, x0, y0, W, H, par, siz);
			}
		const size_t items = seam_items(W, H);
		for (size_t t = 0; t < items; ++t) seam_item(mem, views, b, par, t, W, H);
		for (size_t i = 0; i < L; ++i) rollup_pixel(mem, par, siz, i);
	}
	for (size_t i = 0; i < L; ++i) out[i] = resolve_word(views[i], num_src, min_region, parent.data(), size.data(), L, i);
	return 0;
}

// host/main.cpp's background job: per source a 0 / 255 mask, Connect + Label_Update, the fill rule, the words rebuilt
extern "C" int dvp_clean_selected_views_mirror(const uint32_t* views, int W, int H, int num_src, int min_region, uint32_t* out) {
	if (!views || !out || W < 1 || H < 1 || num_src < 0 || num_src > 32) return 1;
	const int width = W, height = H, nsrc = num_src;
	std::vector<Mat> fill(nsrc);
#pragma omp parallel for schedule(dynamic, 1) num_threads(nsrc < 8 ? (nsrc > 0 ? nsrc : 1) : 8)
	for (int i = 0; i < nsrc; ++i) {
		Mat visible(height, width, CV_8UC1);
		for (int r = 0; r < height; ++r) {
			const uint32_t* w = views + (size_t)r * width;
			uint8_t* v = visible.ptr<uint8_t>(r);
			for (int c = 0; c < width; ++c) v[c] = ((w[c] >> i) & 1u) ? 255 : 0;
		}
		Mat region(height, width, CV_32S);
		std::vector<int> region_size;
		Connect(visible, region, region_size);
		Label_Update(region, region_size);
		fill[i] = Mat(height, width, CV_8UC1);
		for (int r = 0; r < height; ++r) {
			const int* lab = region.ptr<int>(r);
			uint8_t* f = fill[i].ptr<uint8_t>(r);
			for (int c = 0; c < width; ++c) f[c] = (lab[c] != 0 && region_size[lab[c]] >= min_region) ? 0 : 1;
		}
	}
#pragma omp parallel for schedule(static) num_threads(8)
	for (int r = 0; r < height; ++r) {
		uint32_t* w = out + (size_t)r * width;
		for (int c = 0; c < width; ++c) {
			unsigned int mask = 0;
			for (int i = 0; i < nsrc; ++i) mask |= (unsigned int)fill[i].at<uint8_t>(r, c) << i;
			w[c] = mask;
		}
	}
	return 0;
}
