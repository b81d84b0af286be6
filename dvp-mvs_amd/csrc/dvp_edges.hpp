// dvp_edges.hpp — the depth-edge prior (EdgeSegment mode 0: median-adaptive Canny, APD.cpp:404-466; host/edges.cpp) as
// per-pixel functions for the device (dvp_edges.hip) and, the same text, for a serial host build (tests/edges_host).
// All arithmetic is integer apart from one binary32 product for the low threshold.  Stages:
//   1. grey bytes      grey_byte: what convertTo(CV_8UC1) / lrintf + saturate gives (round half to even)
//   2. thresholds      thresholds(): median of the 256-bin histogram over bins 0..254, CannyL2's clamp / square / floor
//   3. + 4. map3_at    Sobel 3x3 (replicated border), mag = gx^2 + gy^2 with a zero frame, sector non-maximum suppression
//                      -> 0 = candidate, 1 = nothing, 2 = strong.  mag is recomputed from the bytes, never stored.
//   5. hysteresis      union-find over the non-empty pixels (uf_find / uf_union / merge_pixel): a candidate is an edge when
//                      its set holds a strong pixel — what the host's stack walk computes, in any order
//   6. frame fix-ups   fixed_at: APD.cpp:452-463 with their sequential meaning, as a function of the map before them
#ifndef DVP_EDGES_HPP_
#define DVP_EDGES_HPP_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DVP_EHD __host__ __device__ inline
#else
#define DVP_EHD inline
#endif

namespace dvpedge {

enum { MAP_CANDIDATE = 0, MAP_NONE = 1, MAP_STRONG = 2 };

// (uint8_t)min(255, max(0, lrintf(v))) under the default rounding mode; what lrintf cannot represent (NaN, |v| >= 2^63) is
// LONG_MIN on the host, so 0
DVP_EHD uint8_t grey_byte(float v) {
	const float r = rintf(v);
	if (!(r > 0.0f) || !(r < 9.2233720368547758e18f)) return 0;
	return r > 255.0f ? (uint8_t)255 : (uint8_t)(int)r;
}

// APD.cpp:428-431 and CannyL2's threshold rules (edges.cpp:14-18): median -1 gives (0, -1), median 0 gives (0, 0)
DVP_EHD void thresholds_of_median(int median, int* low, int* high) {
	const float sigma = 0.67f;
	int t1 = (int)((1 - sigma) * median), t2 = median;
	if (t1 > 32767) t1 = 32767;
	if (t2 > 32767) t2 = 32767;
	*low = t1 > 0 ? t1 * t1 : t1;     // squared only when positive; floor of an integer is itself
	*high = t2 > 0 ? t2 * t2 : t2;
}
// hist: pixels per grey level, pixels = rows * cols (APD.cpp:404-427)
DVP_EHD int median_of(const unsigned* hist, int pixels) {
	const int half = pixels / 2;
	int sum = 0;
	for (int i = 0; i < 255; ++i) {   // bin 255 is never reached: -1 when more than half of the pixels are 255
		sum += (int)hist[i];
		if (sum > half) return i;
	}
	return -1;
}

DVP_EHD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// px(y, x): the grey byte at image coordinates inside [0, H) x [0, W)
template <class Px>
DVP_EHD void sobel(const Px& px, int x, int y, int W, int H, int* gx, int* gy) {
	const int x0 = clampi(x - 1, 0, W - 1), x1 = clampi(x + 1, 0, W - 1), y0 = clampi(y - 1, 0, H - 1), y1 = clampi(y + 1, 0, H - 1);
	const int a = px(y0, x0), b = px(y0, x), c = px(y0, x1), d = px(y, x0), e = px(y, x1), f = px(y1, x0), g = px(y1, x), h = px(y1, x1);
	*gx = (c + 2 * e + h) - (a + 2 * d + f);
	*gy = (f + 2 * g + h) - (a + 2 * b + c);
}
// the magnitude plane with its zero frame
template <class Px>
DVP_EHD int mag_at(const Px& px, int x, int y, int W, int H) {
	if (x < 0 || y < 0 || x >= W || y >= H) return 0;
	int gx, gy;
	sobel(px, x, y, W, H, &gx, &gy);
	return gx * gx + gy * gy;
}
// edges.cpp:43-60
template <class Px>
DVP_EHD uint8_t map3_at(const Px& px, int x, int y, int W, int H, int low, int high) {
	int xs, ys;
	sobel(px, x, y, W, H, &xs, &ys);
	const int m = xs * xs + ys * ys;
	if (m <= low) return MAP_NONE;
	const int TG22 = 13573;   // (int)(tan(22.5 deg) * 2^15 + 0.5)
	const int ax = xs < 0 ? -xs : xs;
	const long long ay = (long long)(ys < 0 ? -ys : ys) << 15;
	const long long tg22x = (long long)ax * TG22;
	bool keep;
	if (ay < tg22x) keep = m > mag_at(px, x - 1, y, W, H) && m >= mag_at(px, x + 1, y, W, H);
	else {
		const long long tg67x = tg22x + ((long long)ax << 16);
		if (ay > tg67x) keep = m > mag_at(px, x, y - 1, W, H) && m >= mag_at(px, x, y + 1, W, H);
		else {
			const int s = (xs ^ ys) < 0 ? -1 : 1;
			keep = m > mag_at(px, x - s, y - 1, W, H) && m > mag_at(px, x + s, y + 1, W, H);
		}
	}
	if (!keep) return MAP_NONE;
	return m > high ? MAP_STRONG : MAP_CANDIDATE;
}

// ---- hysteresis: label equivalence.  parent[i] <= i always, so the links form a forest whose roots are the smallest index
// of their set.  Mem gives the memory operations: device-scope atomics on the GPU (a plain load may be served by an L1 line
// another CU has since written), plain ones in the serial host build.
template <class Mem>
DVP_EHD unsigned uf_find(Mem& mem, unsigned* parent, unsigned x) {
	unsigned p = mem.load(parent + x);
	while (p != x) {
		const unsigned g = mem.load(parent + p);
		if (g != p) mem.min(parent + x, g);   // path halving: x skips its parent (g is in the same set and smaller)
		x = p;
		p = g;
	}
	return x;
}
template <class Mem>
DVP_EHD void uf_union(Mem& mem, unsigned* parent, unsigned a, unsigned b) {
	for (;;) {
		a = uf_find(mem, parent, a);
		b = uf_find(mem, parent, b);
		if (a == b) return;
		if (a < b) { const unsigned t = a; a = b; b = t; }
		const unsigned old = mem.min(parent + a, b);   // a was a root when read: hang it below b
		if (old == a) return;                          // ... and still was: done
		a = old;                                       // somebody hung it elsewhere meanwhile: unite that with b
	}
}
// pixel (x, y) unites with its non-empty forward neighbours E, SW, S, SE
template <class Mem>
DVP_EHD void merge_pixel(Mem& mem, const uint8_t* map3, unsigned* parent, int x, int y, int W, int H) {
	const size_t i = (size_t)y * W + x;
	if (map3[i] == MAP_NONE) return;
	if (x + 1 < W && map3[i + 1] != MAP_NONE) uf_union(mem, parent, (unsigned)i, (unsigned)(i + 1));
	if (y + 1 < H) {
		const size_t j = i + W;
		if (x > 0 && map3[j - 1] != MAP_NONE) uf_union(mem, parent, (unsigned)i, (unsigned)(j - 1));
		if (map3[j] != MAP_NONE) uf_union(mem, parent, (unsigned)i, (unsigned)j);
		if (x + 1 < W && map3[j + 1] != MAP_NONE) uf_union(mem, parent, (unsigned)i, (unsigned)(j + 1));
	}
}

// ---- frame fix-ups (APD.cpp:452-463): raw(y, x) != 0 is the map before them; the column pass, then the row pass on its result
template <class Raw>
DVP_EHD bool fixed_cols(const Raw& raw, int x, int y, int W) {
	if (!raw(y, x)) return false;
	if (x == 0 && !raw(y, 1)) return false;
	if (x == W - 1 && !raw(y, W - 2)) return false;
	return true;
}
template <class Raw>
DVP_EHD uint8_t fixed_at(const Raw& raw, int x, int y, int W, int H) {
	if (!fixed_cols(raw, x, y, W)) return 0;
	if (y == 0 && !fixed_cols(raw, x, 1, W)) return 0;
	if (y == H - 1 && !fixed_cols(raw, x, H - 2, W)) return 0;
	return 255;
}

}   // namespace dvpedge
#endif
