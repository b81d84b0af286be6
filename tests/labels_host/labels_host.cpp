// Host build of the device label prior's steps (dvp-mvs_amd/csrc/dvp_labels.hpp), one launch after the other, one pixel after the
// other, tile by tile where the device uses tiles (TEST INFRASTRUCTURE): lets the CPU tests hold the kernels' arithmetic against
// the host mirror's LabelSegment without a GPU.  Same steps, same order, same words as dvp_labels.hip.  The second export is the
// host mirror itself: host/labels.cpp's LabelSegment with its intermediate maps.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../dvp-mvs_amd/csrc/dvp_labels.hpp"
#include "../../dvp-mvs_amd/csrc/dvp_labels_mid.hpp"
#include "../../dvp-mvs_amd/host/APD.h"

using namespace dvplab;

namespace {
struct HostMem {   // one thread: plain memory operations
	unsigned load(const unsigned* p) const { return *p; }
	unsigned min(unsigned* p, unsigned v) const { const unsigned o = *p; if (v < o) *p = v; return o; }
	unsigned add(unsigned* p, unsigned v) const { const unsigned o = *p; *p = o + v; return o; }
};

// dvp_vc_tiles, dvp_vc_seams, dvp_vc_rollup on plane 0 of a word map
void components(const uint32_t* words, int W, int H, unsigned* parent, unsigned* size) {
	using namespace dvpvc;
	HostMem mem;
	unsigned lab[TILE_PIXELS], cnt[TILE_PIXELS];
	uint64_t rows[TILE_H];
	for (int y0 = 0; y0 < H; y0 += TILE_H)
		for (int x0 = 0; x0 < W; x0 += TILE_W) {
			for (int r = 0; r < TILE_H; ++r) {
				uint64_t clear = 0;
				for (int lane = 0; lane < TILE_W; ++lane) {
					const int x = x0 + lane, y = y0 + r;
					const uint32_t word = (x < W && y < H) ? words[(size_t)y * W + x] : 0xffffffffu;
					if (!(word & 1u)) clear |= (uint64_t)1 << lane;
				}
				for (int lane = 0; lane < TILE_W; ++lane) tile_init(lab, cnt, rows, r, lane, clear);
			}
			for (int r = 0; r < TILE_H; ++r)
				for (int lane = 0; lane < TILE_W; ++lane) tile_union_up(mem, lab, rows, r, lane);
			for (int r = 0; r < TILE_H; ++r)
				for (int lane = 0; lane < TILE_W; ++lane) tile_count(mem, lab, cnt, rows, r, lane);
			for (int r = 0; r < TILE_H; ++r)
				for (int lane = 0; lane < TILE_W; ++lane) tile_store(mem, lab, cnt, rows, r, lane, x0, y0, W, H, parent, size);
		}
	const size_t items = seam_items(W, H), L = (size_t)W * H;
	for (size_t t = 0; t < items; ++t) seam_item(mem, words, 0, parent, t, W, H);
	for (size_t i = 0; i < L; ++i) rollup_pixel(mem, parent, size, i);
}

void resize(const uint8_t* src, size_t pitch, int sw, int sh, uint8_t* dst, int dw, int dh, int thr) {
	const double sx = (double)sw / dw, sy = (double)sh / dh;
	for (int y = 0; y < dh; ++y)
		for (int x = 0; x < dw; ++x) {
			const uint8_t v = resized_byte(src, pitch, sw, sh, sx, sy, x, y);
			dst[(size_t)y * dw + x] = thr < 0 ? v : (v > thr ? 255 : 0);
		}
}
struct WhitePx {
	const uint8_t* map;
	int W;
	bool operator()(int y, int x) const { return map[(size_t)y * W + x] != 0; }
};
void copy_out(void* dst, const void* src, size_t bytes) { if (dst) memcpy(dst, src, bytes); }
}   // namespace

// sizes[7]: quarter cols, rows, level cols, rows, weak_tex_num, unit, 0
extern "C" int dvp_label_sizes_host(int W, int H, int scale, int* sizes) {
	if (W < 1 || H < 1 || scale < 0 || scale > 10) return 1;
	const Geometry g = geometry(W, H, scale);
	const int v[6] = { g.qw, g.qh, g.lw, g.lh, g.weak_tex_num, g.unit };
	memcpy(sizes, v, sizeof(v));
	return 0;
}

// the kernels' text, serially.  Every stage pointer may be NULL.
extern "C" int dvp_label_map_serial(const uint8_t* grey, int W, int H, long long pitch, int scale, int32_t* label_out, uint8_t* quarter_out, uint8_t* texture_out,
                                    int32_t* region_out, uint8_t* lines_out, uint8_t* resized_out, uint8_t* cleaned_out) {
	if (!grey || !label_out || W < 1 || H < 1 || scale < 0 || scale > 10 || pitch < W) return 1;
	const Geometry g = geometry(W, H, scale);
	if (g.qw < 3 || g.qh < 3 || g.lw < 3 || g.lh < 3) return 1;
	const size_t Lq = (size_t)g.qw * g.qh, Ll = (size_t)g.lw * g.lh, Lm = Lq > Ll ? Lq : Ll;
	std::vector<uint8_t> half((size_t)g.hw * g.hh), quarter(Lq), texture(Lq), resized(Ll), cleaned(Ll);
	std::vector<uint32_t> words(Lm);
	std::vector<unsigned> parent(Lm), size(Lm), rank(Ll);
	std::vector<int32_t> region(Lq);
	// part A
	resize(grey, (size_t)pitch, g.W, g.H, half.data(), g.hw, g.hh, -1);
	resize(half.data(), (size_t)g.hw, g.hw, g.hh, quarter.data(), g.qw, g.qh, -1);
	for (int y = 0; y < g.qh; ++y)
		for (int x = 0; x < g.qw; ++x) {
			const size_t i = (size_t)y * g.qw + x;
			texture[i] = texture_at(quarter.data(), g.qw, g.qh, x, y);
			words[i] = texture[i] ? 1u : 0u;
		}
	components(words.data(), g.qw, g.qh, parent.data(), size.data());
	for (size_t i = 0; i < Lq; ++i) region[i] = region_at(words.data(), parent.data(), size.data(), g.weak_tex_num, i);
	copy_out(quarter_out, quarter.data(), Lq);
	copy_out(texture_out, texture.data(), Lq);
	copy_out(region_out, region.data(), Lq * 4);
	// the host middle
	std::vector<unsigned> list;
	std::vector<uint8_t> drawn(Lq, 0);
	dvplabmid::DrawRegionLines(region.data(), g.qw, g.qh, g.unit, [&](int x, int y) {
		const size_t i = (size_t)y * g.qw + x;
		if (!drawn[i]) { drawn[i] = 1; list.push_back((unsigned)i); }
	});
	// part B
	std::vector<uint8_t> lines(texture);
	for (unsigned i : list) lines[i] = 255;
	copy_out(lines_out, lines.data(), Lq);
	resize(lines.data(), (size_t)g.qw, g.qw, g.qh, resized.data(), g.lw, g.lh, ROBERTS_THRESHOLD);
	for (int y = 0; y < g.lh; ++y)
		for (int x = 0; x < g.lw; ++x) {
			const size_t i = (size_t)y * g.lw + x;
			const bool frame = x == 0 || y == 0 || x == g.lw - 1 || y == g.lh - 1;
			cleaned[i] = frame ? cleaned_at(WhitePx{ resized.data(), g.lw }, x, y, g.lw, g.lh) : resized[i];
			words[i] = cleaned[i] ? 1u : 0u;
		}
	copy_out(resized_out, resized.data(), Ll);
	copy_out(cleaned_out, cleaned.data(), Ll);
	components(words.data(), g.lw, g.lh, parent.data(), size.data());
	// block sums, scan of the sums, ranks
	const size_t blocks = (Ll + SCAN_BLOCK - 1) / SCAN_BLOCK;
	std::vector<unsigned> sums(blocks, 0);
	for (size_t b = 0; b < blocks; ++b)
		for (size_t i = b * SCAN_BLOCK; i < Ll && i < (b + 1) * SCAN_BLOCK; ++i) sums[b] += is_root(words.data(), parent.data(), i);
	unsigned carry = 0;
	for (size_t b = 0; b < blocks; ++b) { const unsigned n = sums[b]; sums[b] = carry; carry += n; }
	for (size_t b = 0; b < blocks; ++b) {
		unsigned before = sums[b];
		for (size_t i = b * SCAN_BLOCK; i < Ll && i < (b + 1) * SCAN_BLOCK; ++i)
			if (is_root(words.data(), parent.data(), i)) rank[i] = before++;
	}
	for (size_t i = 0; i < Ll; ++i) label_out[i] = label_at(words.data(), parent.data(), size.data(), rank.data(), g.weak_tex_num, i);
	return 0;
}

// host/labels.cpp: LabelSegment(scale, image, &stages).  threads: the team its resize may use (HostThreads), 0 = as it comes
extern "C" int dvp_label_map_mirror(const uint8_t* grey, int W, int H, long long pitch, int scale, int threads, int32_t* label_out, uint8_t* quarter_out, uint8_t* texture_out,
                                    uint8_t* lines_out, uint8_t* resized_out, uint8_t* cleaned_out) {
	if (!grey || !label_out || W < 1 || H < 1 || scale < 0 || pitch < W) return 1;
	Mat img(H, W, CV_8UC1);
	for (int y = 0; y < H; ++y) memcpy(img.ptr<uint8_t>(y), grey + (size_t)y * pitch, (size_t)W);
	SetThisThreadHostThreads(threads);
	LabelStages st;
	const Mat lab = LabelSegment(scale, img, &st);
	SetThisThreadHostThreads(0);
	auto put = [](void* dst, const Mat& m, size_t elem) {
		if (!dst) return;
		for (int y = 0; y < m.rows; ++y) memcpy((uint8_t*)dst + (size_t)y * m.cols * elem, m.ptr<uint8_t>(y), (size_t)m.cols * elem);
	};
	put(label_out, lab, 4);
	put(quarter_out, st.quarter, 1);
	put(texture_out, st.texture, 1);
	put(lines_out, st.texture_lines, 1);
	put(resized_out, st.resized, 1);
	put(cleaned_out, st.cleaned, 1);
	return 0;
}
