// dvp_cloudprep.hpp — the preparation `apd --evaluate` runs on a cloud before it measures: finite points only, an optional 4 x 4
// transform, an optional crop with a polygon prism, an optional voxel down-sampling, one rounding to binary32.  The same text for the
// device (dvp_cloudprep.hip), the host flavour (host/evaluate.cpp) and the test tool (tests/cloudprep_host).  The definition is the
// project's own; it follows the Tanks and Temples protocol's steps and pins to no other library's bits.
// All arithmetic is binary64 with one rounding per operator (-ffp-contract=off); only the last step rounds to binary32.  Input order
// is kept throughout.
//   finite     a point with a non-finite coordinate is dropped; the others become binary64 exactly
//   transform  16 row-major doubles m, last row exactly 0 0 0 1, all finite: x' = ((m00*x + m01*y) + m02*z) + m03, y' and z' alike;
//              a point whose image has a non-finite coordinate is dropped
//   crop       axis w, (u, v) = (1, 2), (0, 2), (0, 1) for w = 0, 1, 2; kept iff axis_min <= p[w] <= axis_max and an odd number of
//              polygon edges (i, j = (i + 1) % n) have (Vi[v] < p[v] && Vj[v] >= p[v]) || (Vj[v] < p[v] && Vi[v] >= p[v]) and
//              Vi[u] + (p[v] - Vi[v]) / (Vj[v] - Vi[v]) * (Vj[u] - Vi[u]) < p[u]   (left to right; a horizontal edge never crosses)
//   voxel      edge s; per axis lo = the minimum over the kept points, o = lo - s*0.5, t = (p - o) / s, i = floor(t), f = t - i
//              (exact), q = (uint64)floor(f * 2^32).  Key: the three i + 1 packed as dvpce::cell_key packs them.  Per voxel and axis
//              Q = the integer sum of q, n the count, `first` the smallest kept-order index.  Centroid c = o + ((double)i +
//              ((double)Q / (double)n) * 2^-32) * s.  One point per voxel, in ascending `first`.  Integer sums and minima do not
//              depend on the order: the device's atomics give the serial loop's bits.
//   rounding   every output coordinate to binary32 once, to nearest even.  With no option: the finite input points, bit for bit.
#ifndef DVP_CLOUDPREP_HPP_
#define DVP_CLOUDPREP_HPP_

#include "dvp_cloudeval.hpp"

#include <unordered_map>

namespace dvpcp {

constexpr int kMinPolygon = 3, kMaxPolygon = 256;
constexpr long long kMaxKept = 1ll << 30;   // kept points of one cloud that are down-sampled: Q stays below 2^62, a slot fits 32 bits

// parser-independent description of one cloud's preparation
struct Prep {
	bool has_transform = false;
	double m[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
	int crop_axis = -1;                 // -1: no crop
	double axis_min = 0.0, axis_max = 0.0;
	std::vector<double> polygon;        // 3 doubles per vertex
	double voxel = 0.0;                 // 0: no down-sampling
	bool any() const { return has_transform || crop_axis >= 0 || voxel != 0.0; }
};

// what the kernels and the serial loop take per point: the three rows of m, the crop's axes and bounds; the polygon as (u, v) pairs
struct PointRule {
	double m[12];
	int has_transform, crop_axis, u, v, num_polygon;
	double axis_min, axis_max;
};

struct Voxels {
	double o[3], s;
};

DVP_CHD bool finite1(double x) { return (x - x) == 0.0; }

DVP_CHD void transform_point(const double* m, const double p[3], double out[3]) {
	for (int r = 0; r < 3; ++r) out[r] = ((m[4 * r] * p[0] + m[4 * r + 1] * p[1]) + m[4 * r + 2] * p[2]) + m[4 * r + 3];
}

// one polygon edge Vi -> Vj crossed by the ray from p towards smaller u
DVP_CHD bool edge_crossed(double iu, double iv, double ju, double jv, double pu, double pv) {
	if (!((iv < pv && jv >= pv) || (jv < pv && iv >= pv))) return false;
	return iu + (pv - iv) / (jv - iv) * (ju - iu) < pu;
}

DVP_CHD bool inside_crop(const PointRule& r, const double* uv, const double p[3]) {
	if (!(r.axis_min <= p[r.crop_axis] && p[r.crop_axis] <= r.axis_max)) return false;
	const double pu = p[r.u], pv = p[r.v];
	int crossings = 0;
	for (int i = 0; i < r.num_polygon; ++i) {
		const int j = i + 1 == r.num_polygon ? 0 : i + 1;
		crossings += edge_crossed(uv[2 * i], uv[2 * i + 1], uv[2 * j], uv[2 * j + 1], pu, pv);
	}
	return crossings & 1;
}

// index i and fixed-point fraction q of one coordinate
DVP_CHD void voxel_parts(double p, double o, double s, double* i, uint64_t* q) {
	const double t = (p - o) / s;
	*i = floor(t);
	*q = (uint64_t)floor((t - *i) * 4294967296.0);
}

DVP_CHD uint64_t voxel_key(const double i[3]) {   // dvpce::cell_key's packing of axis_index = i + 1
	return (((uint64_t)i[0] + 1u) << 42) | (((uint64_t)i[1] + 1u) << 21) | ((uint64_t)i[2] + 1u);
}

DVP_CHD double voxel_index_of_key(uint64_t key, int axis) { return (double)(((key >> (42 - 21 * axis)) & 0x1fffffu) - 1u); }

DVP_CHD double centroid(double o, double s, double i, uint64_t Q, uint32_t n) {
	return o + (i + ((double)Q / (double)n) * (1.0 / 4294967296.0)) * s;
}

// ---- host part: the argument checks, the serial text ----------------------------------------------------------------------------------

// "" or what is wrong with the description
inline std::string check_prep(const Prep& p) {
	char text[200];
	if (p.has_transform) {
		for (int k = 0; k < 16; ++k)
			if (!finite1(p.m[k])) { snprintf(text, sizeof text, "the transform holds a non-finite entry (%.9g at %d)", p.m[k], k); return text; }
		if (p.m[12] != 0.0 || p.m[13] != 0.0 || p.m[14] != 0.0 || p.m[15] != 1.0) {
			snprintf(text, sizeof text, "the transform's last row must be 0 0 0 1, got %.9g %.9g %.9g %.9g", p.m[12], p.m[13], p.m[14], p.m[15]);
			return text;
		}
	}
	if (p.crop_axis < -1 || p.crop_axis > 2) return "crop_axis must be -1 (no crop), 0, 1 or 2, got " + std::to_string(p.crop_axis);
	if (p.crop_axis >= 0) {
		const long long n = (long long)(p.polygon.size() / 3);
		if (n < kMinPolygon) return "the crop polygon needs at least 3 vertices, got " + std::to_string(n);
		if (n > kMaxPolygon) return "the crop polygon takes at most 256 vertices, got " + std::to_string(n);
		for (double c : p.polygon)
			if (!finite1(c)) return "the crop polygon holds a non-finite coordinate";
		if (!(p.axis_min <= p.axis_max)) {
			snprintf(text, sizeof text, "axis_min (%.9g) must not exceed axis_max (%.9g)", p.axis_min, p.axis_max);
			return text;
		}
	}
	if (!(p.voxel >= 0.0) || !finite1(p.voxel)) {
		snprintf(text, sizeof text, "voxel must be finite and positive, or 0 for none, got %.9g", p.voxel);
		return text;
	}
	return "";
}

// the per-point rule and the polygon's (u, v) pairs of a checked description
inline PointRule point_rule(const Prep& p, std::vector<double>* uv) {
	PointRule r;
	for (int k = 0; k < 12; ++k) r.m[k] = p.m[k];
	r.has_transform = p.has_transform;
	r.crop_axis = p.crop_axis;
	r.u = p.crop_axis == 0 ? 1 : 0;
	r.v = p.crop_axis == 2 ? 1 : 2;
	r.num_polygon = p.crop_axis >= 0 ? (int)(p.polygon.size() / 3) : 0;
	r.axis_min = p.axis_min;
	r.axis_max = p.axis_max;
	uv->clear();
	for (int i = 0; i < r.num_polygon; ++i) {
		uv->push_back(p.polygon[3 * (size_t)i + r.u]);
		uv->push_back(p.polygon[3 * (size_t)i + r.v]);
	}
	return r;
}

inline std::string check_kept(long long kept) {
	if (kept <= kMaxKept) return "";
	return "the cloud holds " + std::to_string(kept) + " points to down-sample; at most " + std::to_string(kMaxKept) + " (2^30) are supported";
}

// the voxel grid over kept points with per-axis minimum lo and maximum hi; "" or the error
inline std::string make_voxels(const double lo[3], const double hi[3], double s, Voxels* vx) {
	vx->s = s;
	for (int a = 0; a < 3; ++a) {
		vx->o[a] = lo[a] - s * 0.5;
		const double cells = floor((hi[a] - vx->o[a]) / s) + 1.0;
		if (!(cells <= (double)dvpce::kMaxCellsPerAxis)) {
			char text[240];
			snprintf(text, sizeof text, "the cloud extends over %.9g along axis %d, which is %.0f voxels of edge %.9g; at most %lld are supported", hi[a] - vx->o[a], a, cells, s,
			         dvpce::kMaxCellsPerAxis);
			return text;
		}
	}
	return "";
}

// One cloud prepared on the host.  out: the prepared points; first_index (may be NULL): the input index of every output point, for
// a voxel that of its first point; counts: finite, after the transform, inside the crop, output points.  "" or the error.
inline std::string serial_prepare(const float* xyz, long long num, const Prep& prep, std::vector<float>* out, std::vector<long long>* first_index, long long counts[4]) {
	const std::string what = check_prep(prep);
	if (!what.empty()) return what;
	std::vector<double> uv;
	const PointRule rule = point_rule(prep, &uv);
	std::vector<double> kept;
	std::vector<long long> source;
	for (int k = 0; k < 4; ++k) counts[k] = 0;
	for (long long i = 0; i < num; ++i) {
		const float* f = xyz + 3 * i;
		if (!dvpce::finite3(f[0], f[1], f[2])) continue;
		++counts[0];
		double p[3] = { (double)f[0], (double)f[1], (double)f[2] };
		if (rule.has_transform) {
			const double in[3] = { p[0], p[1], p[2] };
			transform_point(rule.m, in, p);
			if (!finite1(p[0]) || !finite1(p[1]) || !finite1(p[2])) continue;
		}
		++counts[1];
		if (rule.crop_axis >= 0 && !inside_crop(rule, uv.data(), p)) continue;
		++counts[2];
		kept.insert(kept.end(), p, p + 3);
		source.push_back(i);
	}
	out->clear();
	if (first_index) first_index->clear();
	const long long nk = (long long)source.size();
	if (prep.voxel == 0.0) {
		for (double c : kept) out->push_back((float)c);
		if (first_index) *first_index = source;
		counts[3] = nk;
		return "";
	}
	const std::string many = check_kept(nk);
	if (!many.empty()) return many;
	if (nk == 0) return "";
	double lo[3] = { kept[0], kept[1], kept[2] }, hi[3] = { kept[0], kept[1], kept[2] };
	for (long long k = 1; k < nk; ++k)
		for (int a = 0; a < 3; ++a) {
			const double c = kept[3 * (size_t)k + a];
			if (c < lo[a]) lo[a] = c;
			if (c > hi[a]) hi[a] = c;
		}
	Voxels vx;
	const std::string extent = make_voxels(lo, hi, prep.voxel, &vx);
	if (!extent.empty()) return extent;
	struct Sum { uint64_t Q[3]; uint32_t n; long long first; double i[3]; };
	std::vector<Sum> sums;                          // in the order the voxels are met: ascending `first`
	std::unordered_map<uint64_t, size_t> where;
	for (long long k = 0; k < nk; ++k) {
		double i[3];
		uint64_t q[3];
		for (int a = 0; a < 3; ++a) voxel_parts(kept[3 * (size_t)k + a], vx.o[a], vx.s, &i[a], &q[a]);
		const auto at = where.emplace(voxel_key(i), sums.size());
		if (at.second) sums.push_back(Sum{ { 0, 0, 0 }, 0u, k, { i[0], i[1], i[2] } });
		Sum& s = sums[at.first->second];
		for (int a = 0; a < 3; ++a) s.Q[a] += q[a];
		++s.n;
	}
	for (const Sum& s : sums) {
		for (int a = 0; a < 3; ++a) out->push_back((float)centroid(vx.o[a], vx.s, s.i[a], s.Q[a], s.n));
		if (first_index) first_index->push_back(source[(size_t)s.first]);
	}
	counts[3] = (long long)sums.size();
	return "";
}

}   // namespace dvpcp
#endif
