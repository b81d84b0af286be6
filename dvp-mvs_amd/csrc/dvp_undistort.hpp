// dvp_undistort.hpp — `apd --convert-from ... --undistort on`: a picture taken with one of COLMAP's camera models resampled into the
// pinhole camera with the same fx, fy, cx, cy and the same size, as per-pixel functions for the device (dvp_undistort.hip) and, the
// same text, for the host (`--convert-on host`, tests/undistort_host).  The reference has no such stage (its colmap2mvsnet.py
// expects pictures that `colmap image_undistorter` has made); this is the project's own definition:
//   1. output pixel (x, y):  u = ((x + 0.5) - cx) / fx,  v = ((y + 0.5) - cy) / fy          (COLMAP's pixel centres at +0.5)
//   2. (u', v') = the model's forward distortion of (u, v), its extra parameters in COLMAP's order after f[, fy], cx, cy
//   3. sx = (fx * u' + cx) - 0.5,  sy = (fy * v' + cy) - 0.5
//   4. qx = floor(32 * sx + 0.5), clamped to [-64, 32 * w + 64] before it becomes an integer (qy alike, with h); a NaN gives a zero
//      pixel;  ix = qx >> 5, a = qx & 31, iy = qy >> 5, b = qy & 31
//   5. per channel  ((32-a)(32-b) p(iy,ix) + a(32-b) p(iy,ix+1) + (32-a)b p(iy+1,ix) + ab p(iy+1,ix+1) + 512) >> 10, a tap
//      outside the picture counting as 0: cv::remap(INTER_LINEAR, BORDER_CONSTANT)'s fixed-point rule with its 5 fractional bits
// Binary64 arithmetic is one IEEE rounding per operator (-ffp-contract=off) in the operand order written here.  No library atan:
// libm's and the device's need not agree in the last bit, so atan_nonneg below is built from + - * / and sqrt, which do.
// No output size is chosen and no blank border is cropped (COLMAP's blank_pixels / min_scale / max_scale): the size stays the camera's.
#ifndef DVP_UNDISTORT_HPP_
#define DVP_UNDISTORT_HPP_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DVP_UHD __host__ __device__ inline
#else
#define DVP_UHD inline
#endif

#include <string>

namespace dvpund {

// COLMAP's camera model ids
enum Model {
	SIMPLE_PINHOLE = 0, PINHOLE = 1, SIMPLE_RADIAL = 2, RADIAL = 3, OPENCV = 4, OPENCV_FISHEYE = 5, FULL_OPENCV = 6, FOV = 7, SIMPLE_RADIAL_FISHEYE = 8, RADIAL_FISHEYE = 9,
	THIN_PRISM_FISHEYE = 10, kNumModels = 11
};
struct ModelInfo { const char* name; int num_params; bool single_f; };   // single_f: `f` stands for fx and fy
inline const ModelInfo& model_info(int model) {
	static const ModelInfo table[kNumModels] = {
		{ "SIMPLE_PINHOLE", 3, true }, { "PINHOLE", 4, false }, { "SIMPLE_RADIAL", 4, true }, { "RADIAL", 5, true }, { "OPENCV", 8, false }, { "OPENCV_FISHEYE", 8, false },
		{ "FULL_OPENCV", 12, false }, { "FOV", 5, false }, { "SIMPLE_RADIAL_FISHEYE", 4, true }, { "RADIAL_FISHEYE", 5, true }, { "THIN_PRISM_FISHEYE", 12, false },
	};
	return table[model];
}

struct Camera { int model; double fx, fy, cx, cy, extra[8]; };   // extra: what follows cx, cy in COLMAP's order, the rest 0

// atan(x) for x >= 0.  Three argument halvings, atan x = 2 atan(x / (1 + sqrt(1 + x * x))), leave t <= tan(pi / 16) < 0.2, where
// t - t^3 / 3 + ... - t^19 / 19 is cut off below 0.2^20 / 21 = 5e-16 of t; each halving adds three roundings.  Relative error
// against a correctly rounded atan: below 1e-13 (measured on [0, 16]: tests/test_undistort_host.py).  A t whose square underflows
// comes back as 8 * (x / 8) = x.  NaN stays NaN.
DVP_UHD double atan_nonneg(double x) {
	double t = x;
	for (int k = 0; k < 3; ++k) t = t / (1.0 + sqrt(1.0 + t * t));
	const double z = t * t;
	double p = -1.0 / 19.0;
	p = p * z + 1.0 / 17.0;
	p = p * z - 1.0 / 15.0;
	p = p * z + 1.0 / 13.0;
	p = p * z - 1.0 / 11.0;
	p = p * z + 1.0 / 9.0;
	p = p * z - 1.0 / 7.0;
	p = p * z + 1.0 / 5.0;
	p = p * z - 1.0 / 3.0;
	p = p * z + 1.0;
	return 8.0 * (t * p);
}

// (u, v) -> (u, v) * atan(r) / r, the equidistant mapping in front of the four fisheye models; unchanged at r = 0
DVP_UHD void fisheye_angle(double* u, double* v) {
	const double r = sqrt(*u * *u + *v * *v);
	if (r > 0.0) {
		const double s = atan_nonneg(r) / r;
		*u = *u * s;
		*v = *v * s;
	}
}

// the model's forward distortion: normalised pinhole coordinates -> normalised coordinates in the picture as taken
DVP_UHD void distort(const Camera& c, double u, double v, double* du, double* dv) {
	const double* k = c.extra;
	switch (c.model) {
	case SIMPLE_RADIAL: {
		const double r2 = u * u + v * v, f = 1.0 + k[0] * r2;
		*du = u * f; *dv = v * f;
		return;
	}
	case RADIAL: {
		const double r2 = u * u + v * v, f = 1.0 + k[0] * r2 + k[1] * (r2 * r2);
		*du = u * f; *dv = v * f;
		return;
	}
	case OPENCV:
	case FULL_OPENCV: {
		const double r2 = u * u + v * v, r4 = r2 * r2;
		double rad = 1.0 + k[0] * r2 + k[1] * r4;
		if (c.model == FULL_OPENCV) {
			const double r6 = r4 * r2;
			rad = (rad + k[4] * r6) / (1.0 + k[5] * r2 + k[6] * r4 + k[7] * r6);
		}
		const double uv = u * v;
		*du = u * rad + 2.0 * k[2] * uv + k[3] * (r2 + 2.0 * (u * u));
		*dv = v * rad + 2.0 * k[3] * uv + k[2] * (r2 + 2.0 * (v * v));
		return;
	}
	case SIMPLE_RADIAL_FISHEYE:
	case RADIAL_FISHEYE:
	case OPENCV_FISHEYE: {
		fisheye_angle(&u, &v);
		const double t2 = u * u + v * v;
		double f = 1.0 + k[0] * t2;
		if (c.model != SIMPLE_RADIAL_FISHEYE) f = f + k[1] * (t2 * t2);
		if (c.model == OPENCV_FISHEYE) {
			const double t4 = t2 * t2;
			f = f + k[2] * (t4 * t2) + k[3] * (t4 * t4);
		}
		*du = u * f; *dv = v * f;
		return;
	}
	case THIN_PRISM_FISHEYE: {   // k1, k2, p1, p2, k3, k4, sx1, sy1
		fisheye_angle(&u, &v);
		const double t2 = u * u + v * v, t4 = t2 * t2;
		const double rad = k[0] * t2 + k[1] * t4 + k[4] * (t4 * t2) + k[5] * (t4 * t4);
		const double uv = u * v;
		*du = u + u * rad + 2.0 * k[2] * uv + k[3] * (t2 + 2.0 * (u * u)) + k[6] * t2;
		*dv = v + v * rad + 2.0 * k[3] * uv + k[2] * (t2 + 2.0 * (v * v)) + k[7] * t2;
		return;
	}
	default:   // SIMPLE_PINHOLE, PINHOLE (FOV never gets here: make_camera)
		*du = u; *dv = v;
		return;
	}
}

// step 4 for one axis: false = NaN
DVP_UHD bool quantise(double s, int size, int* i, int* frac) {
	double q = floor(32.0 * s + 0.5);
	if (!(q == q)) return false;
	const double hi = 32.0 * size + 64.0;
	if (q < -64.0) q = -64.0;
	if (q > hi) q = hi;
	const int qi = (int)q;
	*i = qi >> 5;      // (arithmetic: -64 ... -33 give -2, -32 ... -1 give -1)
	*frac = qi & 31;
	return true;
}

// output pixel (x, y) of a w x h picture with `pitch` bytes per row: B, G, R into out[0 .. 2]
DVP_UHD void undistorted_pixel(const Camera& c, const uint8_t* bgr, int w, int h, size_t pitch, int x, int y, uint8_t* out) {
	const double u = ((x + 0.5) - c.cx) / c.fx, v = ((y + 0.5) - c.cy) / c.fy;
	double du, dv;
	distort(c, u, v, &du, &dv);
	const double sx = (c.fx * du + c.cx) - 0.5, sy = (c.fy * dv + c.cy) - 0.5;
	int ix, iy, a, b;
	out[0] = out[1] = out[2] = 0;
	if (!quantise(sx, w, &ix, &a) || !quantise(sy, h, &iy, &b)) return;
	const bool x0 = ix >= 0 && ix < w, x1 = ix + 1 >= 0 && ix + 1 < w, y0 = iy >= 0 && iy < h, y1 = iy + 1 >= 0 && iy + 1 < h;
	if (!((x0 || x1) && (y0 || y1))) return;
	const int w00 = (32 - a) * (32 - b), w01 = a * (32 - b), w10 = (32 - a) * b, w11 = a * b;
	const uint8_t* r0 = bgr + (size_t)(y0 ? iy : 0) * pitch;       // (a row or column that is outside is never read: its taps are 0)
	const uint8_t* r1 = bgr + (size_t)(y1 ? iy + 1 : 0) * pitch;
	const size_t c0 = 3 * (size_t)(x0 ? ix : 0), c1 = 3 * (size_t)(x1 ? ix + 1 : 0);
	for (int ch = 0; ch < 3; ++ch) {
		const int p00 = (y0 && x0) ? r0[c0 + ch] : 0, p01 = (y0 && x1) ? r0[c1 + ch] : 0, p10 = (y1 && x0) ? r1[c0 + ch] : 0, p11 = (y1 && x1) ? r1[c1 + ch] : 0;
		out[ch] = (uint8_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10);
	}
}

// ---- host only: the argument checks and the whole picture, one pixel after the other
// "" = usable; `params` in COLMAP's order for the model
inline std::string check_undistort(const void* bgr, int w, int h, long long pitch, int model, const double* params, int num_params, const void* out) {
	if (!bgr || !params || !out) return "the picture, the parameters and the output are required";
	if (model < 0 || model >= kNumModels) return "unknown camera model " + std::to_string(model);
	const ModelInfo& m = model_info(model);
	if (model == FOV) return "the FOV camera model is not supported (no undistortion is defined for it)";
	if (num_params != m.num_params) return std::string(m.name) + " takes " + std::to_string(m.num_params) + " parameters, not " + std::to_string(num_params);
	if (w < 1 || h < 1 || w > 65535 || h > 65535) return "bad image geometry (sizes of 1 ... 65535)";
	if (pitch < 3ll * w) return "the pitch is below 3 * width bytes";
	return "";
}
// after check_undistort
inline Camera make_camera(int model, const double* params) {
	const ModelInfo& m = model_info(model);
	Camera c{};
	c.model = model;
	const int first = m.single_f ? 3 : 4;
	c.fx = params[0];
	c.fy = m.single_f ? params[0] : params[1];
	c.cx = params[first - 2];
	c.cy = params[first - 1];
	for (int i = first; i < m.num_params; ++i) c.extra[i - first] = params[i];
	return c;
}
// out: h dense rows of 3 * w bytes
inline void undistort_image_serial(const Camera& c, const uint8_t* bgr, int w, int h, size_t pitch, uint8_t* out) {
	for (int y = 0; y < h; ++y)
		for (int x = 0; x < w; ++x) undistorted_pixel(c, bgr, w, h, pitch, x, y, out + ((size_t)y * w + x) * 3);
}

}   // namespace dvpund
#endif
