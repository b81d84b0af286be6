// dvp_cloudscan.hpp — the definition behind `apd --evaluate --against-scans`: ETH3D's observed-space accuracy from range maps of the
// laser scans as their scanners saw them.  The same text for the device (dvp_cloudscan.hip), the host flavour (host/evaluate.cpp) and
// the test tool (tests/cloudscan_host).  The definition is the project's own: it follows the idea of ETH3D's tool (range images of the
// scans seen from the scanner positions), not its code; no beam cones, no per-voxel averaging ("Cloud evaluation").
//   truth      scan s: binary32 points q in the scanner's frame and 16 row-major doubles M_s (all finite, last row exactly 0 0 0 1).
//              g = M_s q by dvpcp::transform_point in binary64, each coordinate rounded once to binary32, whatever q holds.  The truth
//              cloud is every g in scan order, then point order; the scanner stands at o_s = ((float)m03, (float)m13, (float)m23).
//   texel      binary32, one rounding per operator (-ffp-contract=off).  d = x - o_s per coordinate, r2 = (dx*dx + dy*dy) + dz*dz.
//              (x, s) is void if d is not finite3, r2 is not finite or r2 == 0.  Major axis a = 0 if |dx| >= |dy| && |dx| >= |dz|, else
//              1 if |dy| >= |dz|, else 2; face f = 2a + (d_a < 0); (u, v) = (1, 2), (0, 2), (0, 1) as the crop has them; m = |d_a|,
//              su = d_u / m, iu = min(R - 1, (int)floorf((su + 1.0f) * (0.5f * R))), iv alike; texel t = (f*R + iv)*R + iu.
//              R is a power of two, 16 ... 4096: 0.5f * R and the product by it are exact.
//   map        map_s[t] = the minimum r2 over the non-void truth points of scan s in texel t, +inf where there is none.  r2 >= 0: its
//              bit patterns order as unsigned integers, the minimum is an integer minimum and has no order.
//   gap        of a point p: NaN if p has a non-finite coordinate; else the maximum over the scans s with (p, s) not void and
//              map_s[t_s(p)] finite of sqrt(map_s[t_s(p)]) - sqrt(r2_s(p)), the correctly rounded binary32 square root; -inf if there
//              is no such scan.  gap > 0: some scanner measured a surface `gap` behind p along p's direction.
//   counts     with d2 and the tolerances t_k of dvp_cloudeval.hpp: accurate[k] = within_recon[k], free_space[k] = the finite p with
//              !(d2 <= t_k*t_k) && gap > t_k, unobserved[k] = used_recon - accurate[k] - free_space[k].
#ifndef DVP_CLOUDSCAN_HPP_
#define DVP_CLOUDSCAN_HPP_

#include "dvp_cloudeval.hpp"
#include "dvp_cloudprep.hpp"

namespace dvpcs {

constexpr int kMaxScans = 64, kMinCube = 16, kMaxCube = 4096;
constexpr uint32_t kInfBits = 0x7f800000u;

// d = x - o and r2; false: the pair is void
DVP_CHD bool range2(float x, float y, float z, const float o[3], float d[3], float* r2) {
	d[0] = x - o[0]; d[1] = y - o[1]; d[2] = z - o[2];
	*r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
	return dvpce::finite3(d[0], d[1], d[2]) && (*r2 - *r2) == 0.0f && *r2 != 0.0f;
}

DVP_CHD int texel_axis(float s, int R) {
	const int i = (int)floorf((s + 1.0f) * (0.5f * (float)R));
	return i < R - 1 ? i : R - 1;
}

// the texel of a direction d of a non-void pair, below 6 R R
DVP_CHD uint32_t texel_of(const float d[3], int R) {
	const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
	const int a = ax >= ay && ax >= az ? 0 : ay >= az ? 1 : 2;
	const float da = a == 0 ? d[0] : a == 1 ? d[1] : d[2], du = a == 0 ? d[1] : d[0], dv = a == 2 ? d[1] : d[2];   // (selects, not indexed)
	const int f = 2 * a + (da < 0.0f ? 1 : 0);
	const float m = fabsf(da);
	const int iu = texel_axis(du / m, R), iv = texel_axis(dv / m, R);
	return ((uint32_t)f * (uint32_t)R + (uint32_t)iv) * (uint32_t)R + (uint32_t)iu;
}

// the truth point of q under the three rows m of a scan's matrix
DVP_CHD void truth_point(const double* m, float qx, float qy, float qz, float g[3]) {
	const double in[3] = { (double)qx, (double)qy, (double)qz };
	double out[3];
	dvpcp::transform_point(m, in, out);
	g[0] = (float)out[0]; g[1] = (float)out[1]; g[2] = (float)out[2];
}

DVP_CHD float keep_max(float best, float g) { return g > best ? g : best; }

// the correctly rounded binary32 square root.  On the device this is sqrtf under the library's flags (no fast math: hipcc keeps
// binary32 division and square root correctly rounded); this toolchain's __fsqrt_rn is the native, approximate instruction.
DVP_CHD float root(float x) { return sqrtf(x); }

// ---- host part: the argument checks, the serial text ----------------------------------------------------------------------------------

struct Scan {
	const float* xyz = nullptr;
	long long num = 0;
	double m[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
	void scanner(float o[3]) const { o[0] = (float)m[3]; o[1] = (float)m[7]; o[2] = (float)m[11]; }
};

inline size_t map_words(int R) { return (size_t)6 * (size_t)R * (size_t)R; }

inline std::string check_cube(int R) {
	if (R < kMinCube || R > kMaxCube || (R & (R - 1)) != 0) return "cube_size must be a power of two, 16 ... 4096, got " + std::to_string(R);
	return "";
}

// "" or what is wrong with the scans; *total = the number of their points
inline std::string check_scans(const Scan* scans, int num_scans, long long* total) {
	*total = 0;
	if (num_scans < 1 || num_scans > kMaxScans) return "num_scans must be 1 ... 64, got " + std::to_string(num_scans);
	if (!scans) return "the scans are required";
	for (int s = 0; s < num_scans; ++s) {
		const std::string who = "scan " + std::to_string(s) + ": ";
		if (scans[s].num < 0) return who + "a scan holds 0 or more points, got " + std::to_string(scans[s].num);
		if (scans[s].num > 0 && !scans[s].xyz) return who + "the point array is required";
		dvpcp::Prep p;
		p.has_transform = true;
		for (int k = 0; k < 16; ++k) p.m[k] = scans[s].m[k];
		const std::string what = dvpcp::check_prep(p);
		if (!what.empty()) return who + what;
		*total += scans[s].num;
		if (*total > dvpce::kMaxPoints) return "the scans hold 0 ... 2^31 - 1 points together, got more";
	}
	return "";
}

// the truth cloud: 3 floats per scan point, scan after scan
inline void serial_truth(const Scan* scans, int num_scans, std::vector<float>* truth) {
	truth->clear();
	for (int s = 0; s < num_scans; ++s)
		for (long long i = 0; i < scans[s].num; ++i) {
			const float* q = scans[s].xyz + 3 * i;
			float g[3];
			truth_point(scans[s].m, q[0], q[1], q[2], g);
			truth->insert(truth->end(), g, g + 3);
		}
}

// maps: num_scans * 6 R R values of r2 (+inf: no return), from the truth cloud serial_truth made
inline void serial_maps(const Scan* scans, int num_scans, const float* truth, int R, std::vector<float>* maps) {
	maps->assign((size_t)num_scans * map_words(R), INFINITY);
	const float* g = truth;
	for (int s = 0; s < num_scans; ++s) {
		float o[3];
		scans[s].scanner(o);
		float* map = maps->data() + (size_t)s * map_words(R);
		for (long long i = 0; i < scans[s].num; ++i, g += 3) {
			float d[3], r2;
			if (!range2(g[0], g[1], g[2], o, d, &r2)) continue;
			float& cell = map[texel_of(d, R)];
			cell = dvpce::keep_min(cell, r2);
		}
	}
}

inline float gap_of(float x, float y, float z, const Scan* scans, int num_scans, int R, const float* maps) {
	if (!dvpce::finite3(x, y, z)) return NAN;
	float best = -INFINITY;
	for (int s = 0; s < num_scans; ++s) {
		float o[3], d[3], r2;
		scans[s].scanner(o);
		if (!range2(x, y, z, o, d, &r2)) continue;
		const float behind = maps[(size_t)s * map_words(R) + texel_of(d, R)];
		if (behind == INFINITY) continue;
		best = keep_max(best, root(behind) - root(r2));
	}
	return best;
}

inline void serial_gaps(const float* query, long long nq, const Scan* scans, int num_scans, int R, const float* maps, float* gap_out) {
	for (long long i = 0; i < nq; ++i) gap_out[i] = gap_of(query[3 * i], query[3 * i + 1], query[3 * i + 2], scans, num_scans, R, maps);
}

// free_space[k] from the distances and the gaps of the same points (a non-finite point has NaN in both and is in no count)
inline void count_free_space(const float* d2, const float* gap, long long n, const float* tol, int num_tol, long long* free_space) {
	for (int k = 0; k < num_tol; ++k) free_space[k] = 0;
	for (long long i = 0; i < n; ++i)
		for (int k = 0; k < num_tol; ++k) free_space[k] += !(d2[i] <= tol[k] * tol[k]) && gap[i] > tol[k];
}

// The whole evaluation against scans on the host: the truth cloud and the maps of the scans, both clouds prepared (a NULL description
// prepares nothing but the finite test), dvp_cloudeval.hpp's distances and counts, the gaps of the prepared reconstruction and
// free_space.  counts[8]: the four stage counts of recon, then of the truth cloud.  prepared[2] (may be NULL): the prepared clouds;
// d2_recon / gap (may be NULL): per prepared reconstructed point.  "" or the error.
inline std::string serial_evaluate_scans(const float* recon, long long nr, const dvpcp::Prep* prep_recon, const Scan* scans, int num_scans, const dvpcp::Prep* prep_truth, int R,
                                         const float* tol, int num_tol, long long* within_recon, long long* within_truth, long long* used, long long* free_space, long long* counts,
                                         std::vector<float>* prepared, std::vector<float>* d2_recon, std::vector<float>* gap) {
	std::string what = dvpce::check_tolerances(tol, num_tol);
	if (what.empty()) what = check_cube(R);
	long long total = 0;
	if (what.empty()) what = check_scans(scans, num_scans, &total);
	if (!what.empty()) return what;
	std::vector<float> truth, maps, cloud[2], d2, gaps;
	serial_truth(scans, num_scans, &truth);
	serial_maps(scans, num_scans, truth.data(), R, &maps);
	const dvpcp::Prep none;
	what = dvpcp::serial_prepare(recon, nr, prep_recon ? *prep_recon : none, &cloud[0], nullptr, counts);
	if (what.empty()) what = dvpcp::serial_prepare(truth.data(), total, prep_truth ? *prep_truth : none, &cloud[1], nullptr, counts + 4);
	if (!what.empty()) return what;
	const long long n = (long long)(cloud[0].size() / 3);
	d2.resize((size_t)n);
	what = dvpce::serial_evaluate(cloud[0].data(), n, cloud[1].data(), (long long)(cloud[1].size() / 3), tol, num_tol, within_recon, within_truth, used, d2.data(), nullptr);
	if (!what.empty()) return what;
	gaps.resize((size_t)n);
	serial_gaps(cloud[0].data(), n, scans, num_scans, R, maps.data(), gaps.data());
	count_free_space(d2.data(), gaps.data(), n, tol, num_tol, free_space);
	if (prepared) { prepared[0].swap(cloud[0]); prepared[1].swap(cloud[1]); }
	if (d2_recon) d2_recon->swap(d2);
	if (gap) gap->swap(gaps);
	return "";
}

}   // namespace dvpcs
#endif
