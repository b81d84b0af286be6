// Host build of the device level images' per-texel function (dvp-mvs_amd/csrc/dvp_pyramid.hpp), one texel after the other (TEST
// INFRASTRUCTURE): lets the CPU tests hold the kernel's arithmetic against the numpy model and the host mirror's ResizeLinear
// without a GPU.  Same text, same build flags for the arithmetic (-ffp-contract=off) as dvp_pyramid.hip.
#include <stddef.h>
#include <stdint.h>

#include "../../dvp-mvs_amd/csrc/dvp_pyramid.hpp"

// what dvp_pyr_levels stores for one image: out is lw x lh, dense.  Non-zero: bad arguments.
extern "C" int dvp_pyramid_level_serial(const uint8_t* src, long long pitch, int sw, int sh, int pad_w, int pad_h, int lw, int lh, float* out) {
	if (!src || !out || sw < 1 || sh < 1 || pitch < sw || pad_w < 1 || pad_h < 1 || lw < 1 || lh < 1) return 1;
	const double sx = (double)pad_w / lw, sy = (double)pad_h / lh;
	for (int y = 0; y < lh; ++y)
		for (int x = 0; x < lw; ++x) out[(size_t)y * lw + x] = dvppyr::level_texel(src, (size_t)pitch, sw, sh, pad_w, pad_h, sx, sy, x, y);
	return 0;
}
