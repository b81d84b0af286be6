// TEST INFRASTRUCTURE: the format-2 pieces of dvp_dev.hpp built for the host (see Makefile).
#include <vector>
#include "../../dvp-mvs_amd/csrc/dvp_dev.hpp"

using namespace dvp;

namespace {
// one image as the engine holds it: the padded row-pair float plane (Dev::images) and the binary16 tiles (Dev::images16),
// both built from `img` ([H][W]) as upload_planes / dvp_pairs_to_tiles16 build them.  img == nullptr: a padded plane whose
// texels all differ (binary16 value k + 1 at padded texel k), frame included — what no replicated border can hide
struct Planes {
	Dev d{};
	std::vector<float> pairs;
	std::vector<uint32_t> tiles;
	Planes(const float* img, int W, int H) {
		const int pitch = (W + 2 * kImgPad + 63) / 64 * 64, PW = W + 2 * kImgPad, PH = H + 2 * kImgPad;
		std::vector<float> plain((size_t)pitch * PH, 0.0f);
		for (int y = 0; y < PH; ++y)
			for (int x = 0; x < PW; ++x)
				plain[(size_t)y * pitch + x] = img ? img[(size_t)clampi(y - kImgPad, 0, H - 1) * W + clampi(x - kImgPad, 0, W - 1)]
				                                   : half_bits_to_float((uint32_t)(1 + y * PW + x));
		pairs.assign((size_t)pitch * PH * 2, 0.0f);
		for (int y = 0; y < PH; ++y)
			for (int x = 0; x < pitch; ++x) {
				pairs[((size_t)y * pitch + x) * 2] = plain[(size_t)y * pitch + x];
				pairs[((size_t)y * pitch + x) * 2 + 1] = plain[(size_t)(y + 1 < PH ? y + 1 : y) * pitch + x];
			}
		const int tx16 = img16_tiles_x(W), ty16 = img16_tiles_y(H);
		tiles.assign((size_t)tx16 * ty16 * 32, 0xDEADBEEFu);
		for (int tile = 0; tile < tx16 * ty16; ++tile)
			for (int e = 0; e < kT16E * kT16H; ++e) {
				const int ty = tile / tx16, tx = tile - ty * tx16;
				const int sx = std::min(tx * kT16W + (e % kT16E), PW - 1), sy = std::min(ty * kT16H + (e / kT16E), PH - 1);
				uint32_t h;
				(void)tile_pair_rule(pairs[((size_t)sy * pitch + sx) * 2], pairs[((size_t)sy * pitch + sx) * 2 + 1], &h);
				tiles[(size_t)tile * 32 + e] = h;
			}
		d.width = W; d.height = H; d.num_images = 1; d.pitch = pitch;
		d.org = kImgPad * pitch + kImgPad;
		d.plane_stride = (size_t)pitch * PH;
		d.images = pairs.data();
		d.images16 = tiles.data();
		d.img16_tiles_x = tx16;
		d.img16_plane_bytes = (size_t)tx16 * ty16 * 128;
	}
};
template <int SMP>
bool same_footprint(const Dev& d, float x, float y) {
	unsigned o0, o2;
	TapW<SMP> w0, w2;
	tex_coord_t<0, SMP>(d, x, y, &o0, &w0);
	tex_coord_t<2, SMP>(d, x, y, &o2, &w2);
	if (o2 + 8 > d.img16_plane_bytes) return false;
	float q0[4], q2[4], a0, b0, a2, b2;
	load_quad_t<0>(img_plane<0>(d, 0), o0, &q0[0], &q0[1], &q0[2], &q0[3]);
	load_quad_t<2>(img_plane<2>(d, 0), o2, &q2[0], &q2[1], &q2[2], &q2[3]);
	tap_weights(w0, &a0, &b0);
	tap_weights(w2, &a2, &b2);
	return memcmp(q0, q2, sizeof q0) == 0 && memcmp(&a0, &a2, 4) == 0 && memcmp(&b0, &b2, 4) == 0;
}
}

extern "C" {
// the upload rule of one element (tile_pair_rule): bit 0 = not 8-bit exact, bit 1 = not binary16-exact; *h = the pair
unsigned h16_rule(float a, float b, uint32_t* h) { return tile_pair_rule(a, b, h); }
float h16_decode(uint32_t h) { return half_bits_to_float(h); }
// n coordinates (x, y): how many of them give a footprint (texels + weights) of format 2 that differs from the float planes'
int h16_footprints(const float* img, int W, int H, int sampler, const float* xs, const float* ys, int n) {
	const Planes p(img, W, H);
	int bad = 0;
	for (int i = 0; i < n; ++i) bad += sampler ? !same_footprint<1>(p.d, xs[i], ys[i]) : !same_footprint<0>(p.d, xs[i], ys[i]);
	return bad;
}
// every footprint origin (i0, j0) of the padded plane, i0 in [-PAD, W + PAD - 2], j0 in [-PAD, H + PAD - 2], on the plane of
// distinct texels: how many img16_offset footprints differ from tex_offset's in the float planes (-1: an offset leaves the plane)
int h16_offsets(int W, int H) {
	const Planes p(nullptr, W, H);
	int bad = 0;
	for (int j0 = -kImgPad; j0 <= H + kImgPad - 2; ++j0)
		for (int i0 = -kImgPad; i0 <= W + kImgPad - 2; ++i0) {
			const unsigned o0 = tex_offset(p.d.pitch, i0, j0), o2 = img16_offset(p.d.img16_tiles_x, i0, j0);
			if (o2 + 8 > p.d.img16_plane_bytes) return -1;
			float q0[4], q2[4];
			load_quad_t<0>(img_plane<0>(p.d, 0), o0, &q0[0], &q0[1], &q0[2], &q0[3]);
			load_quad_t<2>(img_plane<2>(p.d, 0), o2, &q2[0], &q2[1], &q2[2], &q2[3]);
			bad += memcmp(q0, q2, sizeof q0) != 0;
		}
	return bad;
}
// n integer pixels: how many of them give ref_texel_t<2> != ref_texel_t<0> (clamp-to-edge)
int h16_ref_texels(const float* img, int W, int H, const int* xs, const int* ys, int n) {
	const Planes p(img, W, H);
	int bad = 0;
	for (int i = 0; i < n; ++i) {
		const float a = ref_texel_t<0>(p.d, xs[i], ys[i]), b = ref_texel_t<2>(p.d, xs[i], ys[i]);
		bad += memcmp(&a, &b, 4) != 0;
	}
	return bad;
}
}
