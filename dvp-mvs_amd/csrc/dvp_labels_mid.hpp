// dvp_labels_mid.hpp — the host-only middle of the label prior (EdgeSegment mode 1, APD.cpp:348-401): the outline of every large
// flat region, the progressive probabilistic Hough transform on it, and the lines it finds.  Plain C++ on plain arrays: the host
// mirror (host/labels.cpp) and the engine library (csrc/dvp_labels.hip, between its two device halves) include this one text.
// The transform is sequential — one random generator, a mask that shrinks as segments are found — and runs on a few thousand
// outline points per region.  cv::HoughLinesP and cv::line are third-party arithmetic (OpenCV >= 3.3), restated from their
// documented algorithms (Matas et al.'s PPHT with OpenCV's multiply-with-carry generator; 8-connected Bresenham line).
#ifndef DVP_LABELS_MID_HPP_
#define DVP_LABELS_MID_HPP_

#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>

namespace dvplabmid {

struct Pt { int x, y; };
struct Segment { int x0, y0, x1, y1; };

// key: width x height, >= 0 = the pixel lies in the large region of that key, < 0 = in none.  A pixel belongs to the outline of
// every large region that one of its 4-neighbours lies in and the pixel itself does not.  One raster pass: every list comes out in
// raster order, the order HoughSegments' generator indexes into.  The lists are in order of their region's first outline pixel.
inline std::vector<std::vector<Pt>> RegionOutlines(const int32_t* key, int width, int height) {
	std::vector<std::vector<Pt>> lists;
	std::unordered_map<int32_t, size_t> slot;
	for (int y = 0; y < height; ++y) {
		const int32_t* row = key + (size_t)y * width;
		for (int x = 0; x < width; ++x) {
			const int32_t self = row[x];
			int32_t n[4] = { x > 0 ? row[x - 1] : -1, x + 1 < width ? row[x + 1] : -1, y > 0 ? row[x - width] : -1, y + 1 < height ? row[x + width] : -1 };
			for (int k = 0; k < 4; ++k) {
				if (n[k] < 0 || n[k] == self) continue;
				bool seen = false;
				for (int j = 0; j < k; ++j) seen = seen || n[j] == n[k];
				if (seen) continue;
				auto it = slot.find(n[k]);
				if (it == slot.end()) { it = slot.emplace(n[k], lists.size()).first; lists.emplace_back(); }
				lists[it->second].push_back(Pt{ x, y });
			}
		}
	}
	return lists;
}

// 8-connected line, both end points included, clipped to the image (cv::line, thickness 1); put(x, y) writes one pixel
template <class Put>
inline void draw_line(int width, int height, int x0, int y0, int x1, int y1, const Put& put) {
	const int dx = std::abs(x1 - x0), dy = std::abs(y1 - y0);
	const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
	int err = dx - dy;
	for (;;) {
		if (x0 >= 0 && x0 < width && y0 >= 0 && y0 < height) put(x0, y0);
		if (x0 == x1 && y0 == y1) break;
		const int e2 = 2 * err;
		if (e2 > -dy) { err -= dy; x0 += sx; }
		if (e2 < dx) { err += dx; y0 += sy; }
	}
}

// Progressive probabilistic Hough transform (Matas, Galambos, Kittler) in the shape of cv::HoughLinesP: rho = 1 px, theta = 1
// degree.  `points`: the set pixels of a width x height image in raster order.  Points are visited in random order; each votes
// for its 180 lines; when a bin reaches `threshold` the line is walked from the point in both directions through the mask, gaps
// of up to `max_gap` pixels are bridged, the walked points are removed (their votes withdrawn if the segment is long enough) and
// a segment of at least `min_length` is reported.
inline std::vector<Segment> HoughSegments(int width, int height, const std::vector<Pt>& points, int threshold, int min_length, int max_gap) {
	const int numangle = 180;
	const int numrho = (int)std::lround(((width + height) * 2 + 1) / 1.0);
	std::vector<int> accum((size_t)numangle * numrho, 0);
	std::vector<uint8_t> mask((size_t)width * height, 0);
	std::vector<float> trig((size_t)numangle * 2);
	for (int n = 0; n < numangle; ++n) {
		const double ang = n * (M_PI / 180.0);
		trig[2 * n] = (float)std::cos(ang);
		trig[2 * n + 1] = (float)std::sin(ang);
	}
	std::vector<Pt> pts(points);
	for (const Pt& p : pts) mask[(size_t)p.y * width + p.x] = 1;
	uint64_t state = (uint64_t)-1;   // cv::RNG((uint64)-1), multiply-with-carry
	auto next_u32 = [&]() { state = (uint64_t)(uint32_t)state * 4164903690U + (uint32_t)(state >> 32); return (uint32_t)state; };
	std::vector<Segment> out;
	for (int count = (int)pts.size(); count > 0; --count) {
		const int idx = (int)(next_u32() % (uint32_t)count);
		const Pt point = pts[idx];
		pts[idx] = pts[count - 1];
		if (!mask[(size_t)point.y * width + point.x]) continue;   // already swallowed by an earlier segment
		int max_val = threshold - 1, max_n = 0;
		for (int n = 0; n < numangle; ++n) {
			const int r = (int)std::lround(point.x * trig[2 * n] + point.y * trig[2 * n + 1]) + (numrho - 1) / 2;
			const int val = ++accum[(size_t)n * numrho + r];
			if (max_val < val) { max_val = val; max_n = n; }
		}
		if (max_val < threshold) continue;
		// walk along the line: the major axis advances one pixel per step, the minor one in 16.16 fixed point
		const int shift = 16;
		const float a = -trig[2 * max_n + 1], b = trig[2 * max_n];
		int x0 = point.x, y0 = point.y, dx0, dy0;
		bool xflag;
		if (std::fabs(a) > std::fabs(b)) {
			xflag = true;
			dx0 = a > 0 ? 1 : -1;
			dy0 = (int)std::lround(b * (1 << shift) / std::fabs(a));
			y0 = (y0 << shift) + (1 << (shift - 1));
		} else {
			xflag = false;
			dy0 = b > 0 ? 1 : -1;
			dx0 = (int)std::lround(a * (1 << shift) / std::fabs(b));
			x0 = (x0 << shift) + (1 << (shift - 1));
		}
		Pt line_end[2] = { point, point };
		for (int k = 0; k < 2; ++k) {
			int gap = 0, x = x0, y = y0, dx = dx0, dy = dy0;
			if (k > 0) { dx = -dx; dy = -dy; }
			for (;; x += dx, y += dy) {
				const int i1 = xflag ? x : x >> shift, j1 = xflag ? y >> shift : y;
				if (i1 < 0 || i1 >= width || j1 < 0 || j1 >= height) break;
				if (mask[(size_t)j1 * width + i1]) { gap = 0; line_end[k] = Pt{ i1, j1 }; }
				else if (++gap > max_gap) break;
			}
		}
		const bool good = std::abs(line_end[1].x - line_end[0].x) >= min_length || std::abs(line_end[1].y - line_end[0].y) >= min_length;
		for (int k = 0; k < 2; ++k) {
			int x = x0, y = y0, dx = dx0, dy = dy0;
			if (k > 0) { dx = -dx; dy = -dy; }
			for (;; x += dx, y += dy) {
				const int i1 = xflag ? x : x >> shift, j1 = xflag ? y >> shift : y;
				if (i1 < 0 || i1 >= width || j1 < 0 || j1 >= height) break;
				uint8_t& m = mask[(size_t)j1 * width + i1];
				if (m) {
					if (good)
						for (int n = 0; n < numangle; ++n) {
							const int r = (int)std::lround(i1 * trig[2 * n] + j1 * trig[2 * n + 1]) + (numrho - 1) / 2;
							--accum[(size_t)n * numrho + r];
						}
					m = 0;
				}
				if (i1 == line_end[k].x && j1 == line_end[k].y) break;
			}
		}
		if (good) out.push_back(Segment{ line_end[0].x, line_end[0].y, line_end[1].x, line_end[1].y });
	}
	return out;
}

// The whole middle: lines over the outlines of all large regions of `key`, drawn with put(x, y).  `unit`: Hough threshold, minimum
// length and maximum gap.  Lines only ever add white and every outline comes from `key`, not from the map drawn into: the regions
// are independent, in any order.  Returns the number of regions; *outline_points (unless NULL) the points over all of them.
template <class Put>
inline size_t DrawRegionLines(const int32_t* key, int width, int height, int unit, const Put& put, size_t* outline_points = nullptr) {
	const std::vector<std::vector<Pt>> lists = RegionOutlines(key, width, height);
	size_t points = 0;
	for (const std::vector<Pt>& outline : lists) {
		points += outline.size();
		for (const Segment& s : HoughSegments(width, height, outline, unit, unit, unit)) draw_line(width, height, s.x0, s.y0, s.x1, s.y1, put);
	}
	if (outline_points) *outline_points = points;
	return lists.size();
}

}   // namespace dvplabmid
#endif
