// dvp_prior.hpp — the per-item arithmetic of the monocular-depth plane prior of a FIRST_INIT pass (APD.cpp:24-49, 1326-1422;
// host/prior.cpp), for the device (dvp_prior.hip) and, the same text, for the host mirror and a serial host build
// (tests/prior_host).  The sequential part — the sparse points, the Delaunay triangulation, the triangle list — is
// dvp_prior_mid.hpp.  Every operation has the type the source gives it: binary32 where it computes in float, binary64 where a
// double literal or a double function widens it, one IEEE rounding per operator (-ffp-contract=off, no fma, no reciprocal).
//
// The barycentric sweep of APD.cpp:1333-1347, `for (float p = 0; p < 1.0; p += step) for (float q = 0; q < 1.0 - p; q += step)`:
//   (a) both counters run through ONE float sequence per triangle, s_0 = 0, s_{k+1} = fl32(s_k + step) (accumulated: k * step is
//       another number); row i exists while (double)s_i < 1.0, column j of it while (double)s_j < 1.0 - (double)s_i;
//   (b) the value stored at a pixel, (float)calculateZ(A, B, C, x, y), depends on the triangle and on (x, y) only;
//   (c) of several triangles whose sweeps reach a pixel the last one in list order wins (the loop overwrites).
// So: an owner map (the largest triangle index that reaches the pixel), then one pass over the pixels.
#ifndef DVP_PRIOR_HPP_
#define DVP_PRIOR_HPP_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DVP_PRIOR_EHD __host__ __device__ inline
#else
#define DVP_PRIOR_EHD inline
#endif

namespace dvpprior {

// One triangle of the sweep: integer-truncated corners, the depth ratio at each, the sweep's step (40 bytes).
struct Tri {
	int32_t x1, y1, x2, y2, x3, y3;
	float r1, r2, r3;
	float step;
};
struct P4 { float x, y, z, w; };

// the next element of the counter sequence
DVP_PRIOR_EHD float seq_next(float s, float step) { return s + step; }
// rows of a triangle's sweep = elements s_k with (double)s_k < 1.0; step in (0, 1]
DVP_PRIOR_EHD unsigned seq_count(float step) {
	unsigned n = 0;
	for (float s = 0; s < 1.0; s = seq_next(s, step)) ++n;
	return n;
}
// column j exists in the row of p
DVP_PRIOR_EHD bool column_exists(float p, float q) { return q < 1.0 - p; }

// the pixel of sweep position (p, q): float products of a float and an int, a binary64 third term, float + float, + double,
// truncated (APD.cpp:1336-1337)
DVP_PRIOR_EHD int sweep_coord(float p, float q, int c1, int c2, int c3) { return (int)(p * c1 + q * c2 + (1.0 - p - q) * c3); }

// APD.cpp:24-49
DVP_PRIOR_EHD double triangle_area(const double* A, const double* B, const double* C) {
	return 0.5 * fabs(A[0] * (B[1] - C[1]) + B[0] * (C[1] - A[1]) + C[0] * (A[1] - B[1]));
}
DVP_PRIOR_EHD double calculate_z(const double A[3], const double B[3], const double C[3], double X, double Y) {
	const double P[3] = { X, Y, 0 };
	const double areaABC = triangle_area(A, B, C);
	const double u = triangle_area(P, B, C) / areaABC;
	const double v = triangle_area(P, C, A) / areaABC;
	const double w = triangle_area(P, A, B) / areaABC;
	return u * A[2] + v * B[2] + w * C[2];
}
// what the sweep of triangle t stores at pixel (x, y)
DVP_PRIOR_EHD float rate_of(const Tri& t, int x, int y) {
	const double A[3] = { (double)t.x1, (double)t.y1, t.r1 };
	const double B[3] = { (double)t.x2, (double)t.y2, t.r2 };
	const double C[3] = { (double)t.x3, (double)t.y3, t.r3 };
	return (float)calculate_z(A, B, C, x, y);
}
// the rate map at a pixel of the dep map
DVP_PRIOR_EHD float rate_at(const Tri* tris, int32_t owner, float middle_rate, int x, int y) { return owner < 0 ? middle_rate : rate_of(tris[owner], x, y); }

// The metric depth at working-size pixel (r, c): (255 - raw) / rate at the pixel RescaleMatToTargetSize reads (APD.cpp:1773-1795:
// the ROW index over the WIDTH ratio, the column index over the height ratio, 0 where that falls outside the map).  Equal sizes
// give ratios of 1 and the pixel itself, where the host skips the rescale.
DVP_PRIOR_EHD float working_depth(const float* raw, const float* rate, int cols, int rows, float scale_x, float scale_y, int r, int c) {
	const int o_r = static_cast<int>(r / scale_x);
	const int o_c = static_cast<int>(c / scale_y);
	if (o_r < 0 || o_r >= rows || o_c < 0 || o_c >= cols) return 0.0f;
	const size_t i = (size_t)o_r * cols + o_c;
	return (255 - raw[i]) / rate[i];
}

// APD.cpp:527-534
DVP_PRIOR_EHD void point_3d(const float* K, int x, int y, float depth, float X[3]) {
	X[0] = depth * (x - K[2]) / K[0];
	X[1] = depth * (y - K[5]) / K[4];
	X[2] = depth;
}
// PlanesFromDepth at (x, y) of the W x H depth map (APD.cpp:1365-1422): forward differences of the back-projected depth, the
// cross product in float, cv::normalize's length in binary64 (a zero vector stays zero), turned towards the camera, R^T n.
// Border pixels keep a zero normal and their depth.
DVP_PRIOR_EHD P4 plane_at(const float* dep, int W, int H, const float* K, const float* R, int x, int y) {
	const size_t i = (size_t)y * W + x;
	P4 pl = { 0.0f, 0.0f, 0.0f, dep[i] };
	if (x < 1 || y < 1 || x >= W - 1 || y >= H - 1) return pl;
	float X[3], X_dx[3], X_dy[3];
	point_3d(K, x, y, dep[i], X);
	point_3d(K, x + 1, y, dep[i + 1], X_dx);
	point_3d(K, x, y + 1, dep[i + W], X_dy);
	const float ax = X_dx[0] - X[0], ay = X_dx[1] - X[1], az = X_dx[2] - X[2];
	const float bx = X_dy[0] - X[0], by = X_dy[1] - X[1], bz = X_dy[2] - X[2];
	float n[3] = { ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx };
	const double len = sqrt((double)n[0] * n[0] + (double)n[1] * n[1] + (double)n[2] * n[2]);
	const double inv = len != 0.0 ? 1.0 / len : 0.0;
	n[0] = (float)(n[0] * inv); n[1] = (float)(n[1] * inv); n[2] = (float)(n[2] * inv);
	const float norm = sqrtf(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
	const float vx = X[0] / norm, vy = X[1] / norm, vz = X[2] / norm;
	if (n[0] * vx + n[1] * vy + n[2] * vz > 0.0f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
	pl.x = R[0] * n[0] + R[3] * n[1] + R[6] * n[2];
	pl.y = R[1] * n[0] + R[4] * n[1] + R[7] * n[2];
	pl.z = R[2] * n[0] + R[5] * n[1] + R[8] * n[2];
	return pl;
}

}   // namespace dvpprior
#endif
