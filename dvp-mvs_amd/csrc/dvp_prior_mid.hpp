// dvp_prior_mid.hpp — the host-only, sequential part of the monocular-depth plane prior (APD.cpp:51-80, 1254-1331): the sparse
// points' depth ratios, the Delaunay triangulation and the list of triangles the barycentric sweep runs over.  Plain C++ on plain
// arrays: the host mirror (host/prior.cpp) and the engine library (csrc/dvp_prior.hip, ahead of its kernels) include this one text.
//
// Third-party arithmetic: the reference triangulates with OpenCV's cv::Subdiv2D (OpenCV >= 3.3, README.md:28; not vendored).  Its
// published behaviour is the Delaunay triangulation of the inserted points plus three virtual vertices of an enclosing triangle
// A=(x0+3m, y0), B=(x0, y0+3m), C=(x0-3m, y0-3m), m = max(width, height) of the bounding rectangle; duplicate insertions are
// ignored.  The triangulation is unique for points in general position, so an incremental Bowyer-Watson construction over the same
// vertex set yields the same triangle *set*; the order of the list (which decides the winner where rasterised triangles overlap by
// a pixel) is not pinned.
#ifndef DVP_PRIOR_MID_HPP_
#define DVP_PRIOR_MID_HPP_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <set>
#include <utility>
#include <vector>

#include "dvp_prior.hpp"

namespace dvppriormid {

using dvpprior::Tri;

struct DTri { int a, b, c; double cx, cy, r2; bool alive; };

// > 0 when p lies inside the circumcircle of the counter-clockwise triangle (a, b, c)
inline long double in_circle(const double* a, const double* b, const double* c, const double* p) {
	const long double ax = (long double)a[0] - p[0], ay = (long double)a[1] - p[1];
	const long double bx = (long double)b[0] - p[0], by = (long double)b[1] - p[1];
	const long double cx = (long double)c[0] - p[0], cy = (long double)c[1] - p[1];
	const long double a2 = ax * ax + ay * ay, b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
	return ax * (by * c2 - b2 * cy) - ay * (bx * c2 - b2 * cx) + a2 * (bx * cy - by * cx);
}

inline double orient(const double* a, const double* b, const double* c) {
	return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]);
}

struct Delaunay {
	std::vector<std::array<double, 2>> pts;   // 0..2 = virtual outer vertices
	std::vector<DTri> tris;
	size_t dead = 0;

	void add_tri(int a, int b, int c) {
		if (orient(pts[a].data(), pts[b].data(), pts[c].data()) < 0) std::swap(b, c);
		DTri t{ a, b, c, 0, 0, 0, true };
		const double* A = pts[a].data(); const double* B = pts[b].data(); const double* C = pts[c].data();
		const double bx = B[0] - A[0], by = B[1] - A[1], cx = C[0] - A[0], cy = C[1] - A[1];
		const double d = 2.0 * (bx * cy - by * cx);
		if (std::fabs(d) > 1e-300) {
			const double ux = (cy * (bx * bx + by * by) - by * (cx * cx + cy * cy)) / d;
			const double uy = (bx * (cx * cx + cy * cy) - cx * (bx * bx + by * by)) / d;
			t.cx = A[0] + ux; t.cy = A[1] + uy; t.r2 = ux * ux + uy * uy;
		} else {
			t.r2 = -1.0;   // degenerate: always take the exact predicate
		}
		tris.push_back(t);
	}

	bool circum_contains(const DTri& t, const double* p) const {
		if (t.r2 >= 0.0) {   // cheap filter with a relative safety margin, exact-ish predicate in the band
			const double dx = p[0] - t.cx, dy = p[1] - t.cy, d2 = dx * dx + dy * dy;
			if (d2 > t.r2 * (1.0 + 1e-7)) return false;
			if (d2 < t.r2 * (1.0 - 1e-7)) return true;
		}
		return in_circle(pts[t.a].data(), pts[t.b].data(), pts[t.c].data(), p) > 0.0L;
	}

	void insert(double x, double y) {
		const int pi = (int)pts.size();
		pts.push_back({ x, y });
		const double p[2] = { x, y };
		std::vector<std::pair<int, int>> edges;
		for (auto& t : tris) {
			if (!t.alive || !circum_contains(t, p)) continue;
			t.alive = false;
			dead++;
			edges.emplace_back(t.a, t.b);
			edges.emplace_back(t.b, t.c);
			edges.emplace_back(t.c, t.a);
		}
		// cavity boundary = edges that belong to exactly one removed triangle
		std::vector<std::pair<int, int>> key(edges.size());
		for (size_t i = 0; i < edges.size(); ++i) key[i] = std::minmax(edges[i].first, edges[i].second);
		std::vector<size_t> ord(edges.size());
		for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
		std::sort(ord.begin(), ord.end(), [&](size_t l, size_t r) { return key[l] < key[r]; });
		for (size_t i = 0; i < ord.size();) {
			size_t j = i + 1;
			while (j < ord.size() && key[ord[j]] == key[ord[i]]) ++j;
			if (j - i == 1) add_tri(edges[ord[i]].first, edges[ord[i]].second, pi);
			i = j;
		}
		if (dead > 4096 && dead * 2 > tris.size()) {   // compact
			std::vector<DTri> keep;
			keep.reserve(tris.size() - dead);
			for (const auto& t : tris) if (t.alive) keep.push_back(t);
			tris.swap(keep);
			dead = 0;
		}
	}
};

// APD.cpp:51-80.  xy: n positions (x, y); rates: n.  Points outside [0,cols)x[0,rows) are not inserted; triangle corners are the
// integer-truncated vertex positions; the three rates are looked up by exact coordinate match (the last duplicate's rate wins,
// as the reference's scan does).  Every live triangle in list order, the virtual vertices' included (rate 0); step is left 0.
inline std::vector<Tri> DelaunayCorners(int cols, int rows, int bound_x, int bound_y, int bound_w, int bound_h, const float* xy, const float* rates, size_t n) {
	Delaunay dt;
	const double big = 3.0 * std::max(bound_w, bound_h);
	dt.pts.push_back({ bound_x + big, (double)bound_y });
	dt.pts.push_back({ (double)bound_x, bound_y + big });
	dt.pts.push_back({ bound_x - big, bound_y - big });
	dt.add_tri(0, 1, 2);
	std::vector<int> owner;                     // dt.pts index - 3 -> index into xy
	std::set<std::pair<float, float>> seen;
	for (size_t i = 0; i < n; ++i) {
		const float qx = xy[2 * i], qy = xy[2 * i + 1];
		if (!(qx >= 0 && qx < cols && qy >= 0 && qy < rows)) continue;
		if (!seen.insert({ qx, qy }).second) {
			for (size_t k = 0; k < owner.size(); ++k)
				if (xy[2 * owner[k]] == qx && xy[2 * owner[k] + 1] == qy) owner[k] = (int)i;
			continue;
		}
		owner.push_back((int)i);
		dt.insert(qx, qy);
	}
	std::vector<Tri> results;
	auto corner = [&](int v, int32_t* x, int32_t* y, float* rate) {
		*x = (int)(float)dt.pts[v][0];
		*y = (int)(float)dt.pts[v][1];
		*rate = v >= 3 ? rates[owner[v - 3]] : 0.0f;
	};
	for (const auto& t : dt.tris) {
		if (!t.alive) continue;
		Tri tri{};
		corner(t.a, &tri.x1, &tri.y1, &tri.r1);
		corner(t.b, &tri.x2, &tri.y2, &tri.r2);
		corner(t.c, &tri.x3, &tri.y3, &tri.r3);
		results.push_back(tri);
	}
	return results;
}

// APD.cpp:536-546 on plain arrays (K, R: 3 x 3 row-major; t: 3)
inline void ProjectPoint(const float* X, const float* K, const float* R, const float* t, float* px, float* py, float* depth) {
	const float tx = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
	const float ty = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
	const float tz = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
	*depth = K[6] * tx + K[7] * ty + K[8] * tz;
	*px = (K[0] * tx + K[1] * ty + K[2] * tz) / *depth;
	*py = (K[3] * tx + K[4] * ty + K[5] * tz) / *depth;
}

// The three skip rules of the sweep (APD.cpp:1326-1331 and the two guards of host/prior.cpp) and its step: false = the triangle
// is not swept — a corner outside the map; three corners on one pixel (step would be inf); collinear integer corners (0/0 in
// calculateZ).  *rule (unless NULL): 0 = swept, 1 ... 3 = the rule that fired.
inline bool SweepStep(int cols, int rows, Tri* t, int* rule = nullptr) {
	auto inside = [&](int x, int y) { return 0 <= x && x < cols && 0 <= y && y < rows; };
	if (rule) *rule = 1;
	if (!(inside(t->x1, t->y1) && inside(t->x2, t->y2) && inside(t->x3, t->y3))) return false;
	const float L01 = sqrt(pow(t->x1 - t->x2, 2) + pow(t->y1 - t->y2, 2));
	const float L02 = sqrt(pow(t->x1 - t->x3, 2) + pow(t->y1 - t->y3, 2));
	const float L12 = sqrt(pow(t->x2 - t->x3, 2) + pow(t->y2 - t->y3, 2));
	const float max_edge_length = std::max(L01, std::max(L02, L12));
	if (rule) *rule = 2;
	if (!(max_edge_length > 0.0f)) return false;
	t->step = 1.0 / max_edge_length;
	const double A[3] = { (double)t->x1, (double)t->y1, t->r1 };
	const double B[3] = { (double)t->x2, (double)t->y2, t->r2 };
	const double C[3] = { (double)t->x3, (double)t->y3, t->r3 };
	if (rule) *rule = 3;
	if (!(dvpprior::triangle_area(A, B, C) > 0.0)) return false;
	if (rule) *rule = 0;
	return true;
}

// The whole host part.  raw: the relative map as read from dep/<id>.dmb (cols x rows floats, dense); xy, xyz: n sparse points
// (2 and 3 floats each, one per sfm/<id>.txt line); K, R, t: the camera as read from cams/<id>_cam.txt (unscaled,
// APD.cpp:1258-1260).  A point counts when it projects to 0 < ix < cols, 0 < iy < rows; its rate is (255 - raw(iy, ix)) over the
// projected depth.  *middle_rate = rates[n / 2] (the middle element, not a median): the rate map outside every triangle.
// tris: the swept triangles in list order; skipped (unless NULL): how often each skip rule fired.  false: an empty map or no
// usable point (the reference indexes rates[0] of an empty vector there).
inline bool PriorTriangles(const float* raw, int cols, int rows, const float* xy, const float* xyz, size_t n, const float* K, const float* R, const float* t,
                           float* middle_rate, std::vector<Tri>* tris, size_t skipped[3] = nullptr) {
	tris->clear();
	if (!raw || cols < 1 || rows < 1) return false;
	std::vector<float> xy_temps, rates;
	for (size_t i = 0; i < n; i++) {
		float px, py, proj_depth;
		ProjectPoint(xyz + 3 * i, K, R, t, &px, &py, &proj_depth);
		const int ix = int(px + 0.5f), iy = int(py + 0.5f);
		if (ix > 0 && ix < cols && iy > 0 && iy < rows) {
			rates.push_back((255 - raw[(size_t)iy * cols + ix]) / proj_depth);
			xy_temps.push_back(xy[2 * i]);
			xy_temps.push_back(xy[2 * i + 1]);
		}
	}
	if (rates.empty()) return false;
	*middle_rate = rates[rates.size() / 2];
	if (skipped) skipped[0] = skipped[1] = skipped[2] = 0;
	for (Tri& tri : DelaunayCorners(cols, rows, 0, 0, cols, rows, xy_temps.data(), rates.data(), rates.size())) {
		int rule = 0;
		if (SweepStep(cols, rows, &tri, &rule)) tris->push_back(tri);
		else if (skipped) skipped[rule - 1]++;
	}
	return true;
}

}   // namespace dvppriormid
#endif
