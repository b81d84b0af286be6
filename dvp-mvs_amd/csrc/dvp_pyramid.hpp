// dvp_pyramid.hpp — a pyramid level's float image as a function of the decoded 8-bit file (host/APD.cpp load_image), one texel at
// a time, for the device (dvp_pyramid.hip) and, the same text, for a serial host build (tests/pyramid_host).  The byte image
// (sw x sh, `pitch` bytes per row) lies at the origin of a pad_w x pad_h canvas — zero beyond the image, cropped beyond the canvas
// (APD.cpp:1059, 1071-1079) — the canvas becomes float and cv::resize(INTER_LINEAR) (host/io.cpp ResizeLinear) takes it to the
// level size.  Binary32 arithmetic is one IEEE rounding per operator (-ffp-contract=off, no fmaf); the source coordinate is formed
// in double (dvp_labels.hpp source_of).
#ifndef DVP_PYRAMID_HPP_
#define DVP_PYRAMID_HPP_

#include <stddef.h>
#include <stdint.h>

#include "dvp_labels.hpp"

namespace dvppyr {

// the canvas at (x, y), 0 <= x < pad_w, 0 <= y < pad_h
DVP_EHD float canvas_at(const uint8_t* src, size_t pitch, int sw, int sh, int x, int y) {
	return (x < sw && y < sh) ? (float)src[(size_t)y * pitch + x] : 0.0f;
}
// The level texel at (dx, dy); sx = (double)pad_w / level_w, sy = (double)pad_h / level_h.  The second tap is clamped to the
// canvas, not to the image: a tap past the image's edge reads the zero padding.  Equal sizes give a zero fraction and the byte,
// where the host skips ResizeLinear: the identity needs no case of its own.
DVP_EHD float level_texel(const uint8_t* src, size_t pitch, int sw, int sh, int pad_w, int pad_h, double sx, double sy, int dx, int dy) {
	int ix, ix1, iy, iy1;
	float a, fy;
	dvplab::source_of(dx, sx, pad_w, &ix, &ix1, &a);
	dvplab::source_of(dy, sy, pad_h, &iy, &iy1, &fy);
	const float h0 = canvas_at(src, pitch, sw, sh, ix, iy) * (1.f - a) + canvas_at(src, pitch, sw, sh, ix1, iy) * a;
	const float h1 = canvas_at(src, pitch, sw, sh, ix, iy1) * (1.f - a) + canvas_at(src, pitch, sw, sh, ix1, iy1) * a;
	return h0 * (1.f - fy) + h1 * fy;
}

}   // namespace dvppyr
#endif
