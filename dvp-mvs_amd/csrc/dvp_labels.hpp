// dvp_labels.hpp — the label prior (EdgeSegment mode 1, APD.cpp:348-401, 437-499; host/labels.cpp) as per-pixel functions for the
// device (dvp_labels.hip) and, the same text, for a serial host build (tests/labels_host).  The result is LabelSegment(scale,
// image)'s CV_32SC1 map, value for value.  Stages:
//   A1  resized_byte    cv::resize(INTER_LINEAR) of bytes through float (host/io.cpp ResizeLinear) + lrintf + saturate, twice:
//                       full -> half -> quarter size
//   A2  texture_at      Roberts cross on the interior, 50 / 50 on the frame, (uchar) of the root, threshold 4: 255 = textured
//   A3  region_at       4-connected components of the black pixels with their sizes (dvp_viewclean.hpp's tile labelling, seam merge
//                       and roll-up on a one-plane word map: word = 1 where the pixel is white); the root index where the
//                       component has at least weak_tex_num pixels, else -1
//   --  the host draws lines into the texture map (dvp_labels_mid.hpp)
//   B1  resized_byte    to the level size, then the threshold 4 again
//   B2  cleaned_at      the frame clean-up of labels.cpp with its sequential meaning, as a function of the map before it
//   B3  is_root / label_at   components at level size; numbers 1, 2, ... in raster order of the components' first pixels (an
//                       exclusive prefix sum over the root flags: block sums, scan of the sums, ranks); 0 = white, -1 = a
//                       component of at most weak_tex_num pixels
// Binary32 arithmetic is one IEEE rounding per operator (-ffp-contract=off, no fmaf); the source coordinate is formed in double.
#ifndef DVP_LABELS_HPP_
#define DVP_LABELS_HPP_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "dvp_edges.hpp"
#include "dvp_viewclean.hpp"

namespace dvplab {

using dvpedge::grey_byte;

enum { ROBERTS_THRESHOLD = 4, SCAN_BLOCK = 1024 };

// the quantities LabelSegment derives from the image size
struct Geometry {
	int W, H, scale;   // the full-size image
	int hw, hh;        // after the first halving
	int qw, qh;        // quarter size
	int lw, lh;        // level size
	int weak_tex_num, unit;
};
inline Geometry geometry(int W, int H, int scale) {
	Geometry g;
	g.W = W; g.H = H; g.scale = scale;
	g.weak_tex_num = (int)(1.0 * H * W / (1024 << scale << scale));
	g.hw = W / 2; g.hh = H / 2;
	g.qw = g.hw / 2; g.qh = g.hh / 2;
	g.unit = (int)((g.qw < g.qh ? g.qw : g.qh) / 30.0);
	const float factor = 1.0f / (float)(1 << scale);
	g.lw = (int)roundf(W * factor);
	g.lh = (int)roundf(H * factor);
	return g;
}

// ResizeLinear's source coordinate of destination index d: (float)((d + 0.5) * s - 0.5) with s = (double)src_n / dst_n, floor, and
// the two clamps that zero the fraction
DVP_EHD void source_of(int d, double s, int src_n, int* i0, int* i1, float* a) {
	float f = (float)((d + 0.5) * s - 0.5);
	int i = (int)floorf(f);
	f -= i;
	if (i < 0) { i = 0; f = 0; }
	if (i >= src_n - 1) { i = src_n - 1; f = 0; }
	*i0 = i;
	*i1 = i + 1 < src_n - 1 ? i + 1 : src_n - 1;
	*a = f;
}
// resize_u8 at destination (dx, dy): the horizontal pass on two rows, then the vertical one, in float; round to nearest (ties to
// even), saturate.  Equal sizes give s = 1, a zero fraction and the source byte: the identity needs no case of its own.
DVP_EHD uint8_t resized_byte(const uint8_t* src, size_t pitch, int sw, int sh, double sx, double sy, int dx, int dy) {
	int ix, ix1, iy, iy1;
	float a, fy;
	source_of(dx, sx, sw, &ix, &ix1, &a);
	source_of(dy, sy, sh, &iy, &iy1, &fy);
	const uint8_t* r0 = src + (size_t)iy * pitch;
	const uint8_t* r1 = src + (size_t)iy1 * pitch;
	const float h0 = (float)r0[ix] * (1.f - a) + (float)r0[ix1] * a;
	const float h1 = (float)r1[ix] * (1.f - a) + (float)r1[ix1] * a;
	return grey_byte(h0 * (1.f - fy) + h1 * fy);
}

// ((uchar)sqrt(t1^2 + t2^2)) > 4 in integers: v = t1^2 + t2^2 <= 130050; the byte cast wraps, so roots 256 ... 260 are black
DVP_EHD bool roberts_white(int v) { return (v >= 25 && v < 65536) || v >= 68121; }
DVP_EHD uint8_t texture_at(const uint8_t* q, int W, int H, int x, int y) {
	int t1 = 50, t2 = 50;
	if (y > 0 && y < H - 1 && x > 0 && x < W - 1) {
		const size_t i = (size_t)y * W + x;
		t1 = (int)q[i] - (int)q[i + W + 1];
		t2 = (int)q[i + W] - (int)q[i + 1];
	}
	return roberts_white(t1 * t1 + t2 * t2) ? (uint8_t)255 : (uint8_t)0;
}

// After dvp_viewclean.hpp's steps 1-3 on the one-plane word map (no unions run any more): the root of a black pixel
DVP_EHD unsigned root_of(const unsigned* parent, size_t i) {
	unsigned x = (unsigned)i, p = parent[x];
	while (p != x) { x = p; p = parent[x]; }
	return x;
}
// A3: the root index where the pixel is black and its component has at least weak_tex_num pixels, else -1
DVP_EHD int32_t region_at(const uint32_t* words, const unsigned* parent, const unsigned* size, int weak_tex_num, size_t i) {
	if (words[i] & 1u) return -1;
	const unsigned r = root_of(parent, i);
	return (long long)size[r] < (long long)weak_tex_num ? -1 : (int32_t)r;
}

// B2 (labels.cpp: the column pass, then the row pass on its result): a frame pixel becomes 0 when its inner neighbour is 0.
// white(y, x): the map before the clean-up is 255 there.  W, H >= 3.
template <class Map>
DVP_EHD bool cleaned_cols(const Map& white, int x, int y, int W) {
	if (!white(y, x)) return false;
	if (x == 0 && !white(y, 1)) return false;
	if (x == W - 1 && !white(y, W - 2)) return false;
	return true;
}
template <class Map>
DVP_EHD uint8_t cleaned_at(const Map& white, int x, int y, int W, int H) {
	if (!cleaned_cols(white, x, y, W)) return 0;
	if (y == 0 && !cleaned_cols(white, x, 1, W)) return 0;
	if (y == H - 1 && !cleaned_cols(white, x, H - 2, W)) return 0;
	return 255;
}

// B3.  A component's root is its first pixel in raster order: Connect's numbers are 1 + the roots before it
DVP_EHD unsigned is_root(const uint32_t* words, const unsigned* parent, size_t i) { return (!(words[i] & 1u) && parent[i] == (unsigned)i) ? 1u : 0u; }
// rank[r]: the number of roots before root r (written at roots only)
DVP_EHD int32_t label_at(const uint32_t* words, const unsigned* parent, const unsigned* size, const unsigned* rank, int weak_tex_num, size_t i) {
	if (words[i] & 1u) return 0;
	const unsigned r = root_of(parent, i);
	return (long long)size[r] <= (long long)weak_tex_num ? -1 : (int32_t)(rank[r] + 1u);
}

}   // namespace dvplab
#endif
