// dvp_cloudicp.hpp — the definition behind `apd --evaluate --refine-alignment`: point-to-point ICP that refines the 4 x 4 matrix which
// brings the reconstruction onto the ground truth, in stages (voxel v, distance d, iterations k) as the Tanks and Temples protocol
// runs them.  The same text for the device (dvp_cloudicp.hip), the host flavour (host/evaluate.cpp) and the test tool
// (tests/cloudicp_host).  The definition is the project's own and pins to no other library's bits.  All arithmetic is binary64 with
// one rounding per operator (-ffp-contract=off); only the distance is dvp_cloudeval.hpp's binary32 sq_dist.
//   step      sources p_i (binary32, index order), targets q_j (binary32, all finite), an increment D (16 row-major doubles, last row
//             exactly 0 0 0 1), a maximum distance d (binary32; d2max = d*d in binary32, a normal number)
//     image       p'_i = ((D00*x + D01*y) + D02*z) + D03, y and z alike (dvpcp::transform_point); r_i = p'_i rounded to binary32.  A
//                 source with a non-finite coordinate, or whose r_i is not finite, has no correspondence.
//     nearest     j(i) = the target that minimises e = sq_dist(r_i, q_j), the smallest j among equal minima; e_i that minimum;
//                 source i corresponds iff e_i <= d2max
//     reference   per axis c = lo + (hi - lo) * 0.5 of the targets' binary32 bounds taken as doubles (0 without targets)
//     leaves      for a corresponding i: a = p'_i - c, b = (double)q_j(i) - c; 16 doubles: a (3), b (3), a_r * b_c (9, row-major),
//                 (double)e_i.  Every other index, padding included: +0.0 sixteen times.
//     sums        each of the 16 is the balanced pairwise tree over the indices 0 ... N - 1, N the power of two >= max(n_src, 1):
//                 S(lo, 1) = leaf(lo), S(lo, n) = S(lo, n/2) + S(lo + n/2, n/2).  The count of correspondences is an integer.
//                 IEEE addition commutes, so a wave's xor-butterfly over 64 consecutive indices is the first six levels, four waves
//                 through LDS two more, further launches over the work-groups' partials the rest: the device's bits are the host's.
//   solve     n >= 3 correspondences: mu_a = Sa / n, mu_b = Sb / n, H_rc = Sab_rc - (Sa_r * Sb_c) / n.  Horn's symmetric matrix
//                 N = | Hxx+Hyy+Hzz  Hyz-Hzy      Hzx-Hxz      Hxy-Hyx     |
//                     | Hyz-Hzy      Hxx-Hyy-Hzz  Hxy+Hyx      Hzx+Hxz     |      (every sum left to right)
//                     | Hzx-Hxz      Hxy+Hyx      -Hxx+Hyy-Hzz Hyz+Hzy     |
//                     | Hxy-Hyx      Hzx+Hxz      Hyz+Hzy      -Hxx-Hyy+Hzz|
//             its dominant eigenvector by cyclic Jacobi sweeps (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3): for A_pq != 0
//             theta = (A_qq - A_pp) / (2 A_pq), t = sign(theta) / (|theta| + sqrt(theta*theta + 1)), c = 1 / sqrt(t*t + 1), s = t*c,
//             columns p, q of A and of V, then rows p, q of A, rotated by (c, s).  Before every sweep off = the sum of A_pq^2 over
//             p < q and dia = the sum of A_pp^2: stop when off <= 2^-106 * dia (off == 0 included), after 30 sweeps at the latest.
//             The eigenvector of the largest A_pp (the first among equals) is q = (w, x, y, z), divided by its norm;
//                 R = | ww+xx-yy-zz  2(xy-wz)     2(xz+wy)    |
//                     | 2(xy+wz)     ww-xx+yy-zz  2(yz-wx)    |      (sums left to right)
//                     | 2(xz-wy)     2(yz+wx)     ww-xx-yy+zz |
//             t = (mu_b + c) - R (mu_a + c), R's row summed as the transform sums it.  E = [R t], D <- E * D with
//             (E D)_rc = ((E_r0*D_0c + E_r1*D_1c) + E_r2*D_2c) + E_r3*D_3c for the three upper rows.  Rigid only, no scale.
//   stage     src = prepare(recon, transform M, crop, voxel v), tgt = prepare(truth, crop, voxel v) (dvp_cloudprep.hpp, v = 0: no
//             down-sampling); D = I; up to k steps: the sums of D, fitness = n / n_src (0 for no source), rmse = sqrt(Se / n) (0 for
//             n = 0), one log record; the stage ends with fewer than 3 correspondences (the record's n says so), or from the second
//             step on when |fitness - previous| < 1e-6 and |rmse - previous| < 1e-6 (Open3D's default criteria, which the protocol's
//             script uses); else D <- E * D.  After the stage M <- D * M.
//   search    a uniform grid over the targets with cell edge h = (double)d * (1 + 2^-10) / R and the (2R + 1)^3 cells around the
//             source's cell, R = 1 or 2; origin = the targets' minimum - (2R + 1) h per axis.  A rounded e <= d2max implies a true
//             per-axis difference below d (1 + 2^-22), which is less than R h by more than the rounding of the two quotients, so the
//             cell indices of such a pair differ by at most R ("Cloud evaluation").  A source whose index along some axis
//             is below R or above the targets' largest + R is more than R cells from every target: no correspondence, not searched.
//             The result does not depend on the visiting order: it is the brute-force loop's, bit for bit.
#ifndef DVP_CLOUDICP_HPP_
#define DVP_CLOUDICP_HPP_

#include <stdlib.h>

#include "dvp_cloudprep.hpp"

namespace dvpci {

constexpr int kMaxStages = 8, kMaxIterations = 1000, kSweepCap = 30;
constexpr uint32_t kNoTarget = 0xffffffffu;

struct Stage {
	double voxel, max_distance;
	int max_iterations;
};

struct LogRecord {   // (the layout of dvp_icp_log)
	int stage, step;
	long long n_src, n;
	double rmse;
};

// the search grid of one stage: a source is searched iff R <= floor((x - origin) / h) <= t_max along every axis
struct Cells {
	dvpce::Grid g;
	double t_max[3];
	int R;
};

DVP_CHD bool searched(const Cells& c, float x, float y, float z) {
	const double p[3] = { (double)x, (double)y, (double)z };
	for (int a = 0; a < 3; ++a) {
		const double t = floor((p[a] - c.g.origin[a]) / c.g.h);
		if (!((double)c.R <= t && t <= c.t_max[a])) return false;
	}
	return true;
}

// the key of neighbour n = 0 ... (2R + 1)^3 - 1 of a searched source's cell: its indices are at least R, so nothing borrows
DVP_CHD uint64_t neighbour_of(uint64_t key, int n, int R) {
	const int W = 2 * R + 1;
	const int64_t dx = n / (W * W) - R, dy = (n / W) % W - R, dz = n % W - R;
	return (uint64_t)((int64_t)key + dx * ((int64_t)1 << 42) + dy * ((int64_t)1 << 21) + dz);
}

DVP_CHD bool closer(float e, uint32_t j, float best, uint32_t best_j) { return e < best || (e == best && j < best_j); }

// p' of a source and its rounding; false: no correspondence whatever the targets
DVP_CHD bool image_of(const double* D, float x, float y, float z, double p[3], float r[3]) {
	const double in[3] = { (double)x, (double)y, (double)z };
	dvpcp::transform_point(D, in, p);
	for (int a = 0; a < 3; ++a) r[a] = (float)p[a];
	return dvpce::finite3(x, y, z) && dvpce::finite3(r[0], r[1], r[2]);
}

DVP_CHD void leaf_of(const double p[3], float qx, float qy, float qz, const double c[3], float e, double leaf[16]) {
	const double q[3] = { (double)qx, (double)qy, (double)qz };
	for (int r = 0; r < 3; ++r) { leaf[r] = p[r] - c[r]; leaf[3 + r] = q[r] - c[r]; }
	for (int r = 0; r < 3; ++r)
		for (int k = 0; k < 3; ++k) leaf[6 + 3 * r + k] = leaf[r] * leaf[3 + k];
	leaf[15] = (double)e;
}

// ---- host part: the argument checks, the serial step, the solve, the stage loop ------------------------------------------------------

inline long long padded(long long n) {
	long long N = 1;
	while (N < n) N <<= 1;
	return N;
}

inline std::string check_distance(float d) {
	const float d2 = d * d;
	if (d > 0.0f && (d - d) == 0.0f && (d2 - d2) == 0.0f && d2 >= 1.17549435e-38f) return "";
	char text[160];
	snprintf(text, sizeof text, "max_distance (%.9g) must be finite and positive with a normal binary32 square", (double)d);
	return text;
}

inline std::string check_increment(const double* D) {
	char text[200];
	for (int k = 0; k < 16; ++k)
		if (!dvpcp::finite1(D[k])) { snprintf(text, sizeof text, "the increment holds a non-finite entry (%.9g at %d)", D[k], k); return text; }
	if (D[12] != 0.0 || D[13] != 0.0 || D[14] != 0.0 || D[15] != 1.0) {
		snprintf(text, sizeof text, "the increment's last row must be 0 0 0 1, got %.9g %.9g %.9g %.9g", D[12], D[13], D[14], D[15]);
		return text;
	}
	return "";
}

inline std::string check_stages(const Stage* stages, int num_stages) {
	if (num_stages < 1 || num_stages > kMaxStages) return "num_stages must be 1 ... 8, got " + std::to_string(num_stages);
	char text[200];
	for (int s = 0; s < num_stages; ++s) {
		const std::string at = "stage " + std::to_string(s) + ": ";
		if (!(stages[s].voxel >= 0.0) || !dvpcp::finite1(stages[s].voxel)) {
			snprintf(text, sizeof text, "voxel must be finite and positive, or 0 for none, got %.9g", stages[s].voxel);
			return at + text;
		}
		const std::string what = check_distance((float)stages[s].max_distance);
		if (!what.empty()) return at + what;
		if (stages[s].max_iterations < 1 || stages[s].max_iterations > kMaxIterations) return at + "max_iterations must be 1 ... 1000, got " + std::to_string(stages[s].max_iterations);
	}
	return "";
}

inline std::string check_targets(const dvpce::Bounds& b, long long num) {
	if (b.finite == num) return "";
	return "the targets must have finite coordinates, " + std::to_string(num - b.finite) + " of " + std::to_string(num) + " have not";
}

inline void reference_point(const dvpce::Bounds& b, double c[3]) {
	for (int a = 0; a < 3; ++a) c[a] = b.finite ? (double)b.lo[a] + ((double)b.hi[a] - (double)b.lo[a]) * 0.5 : 0.0;
}

// the search grid over targets within `b` (all finite); "" or the error
inline std::string make_cells(const dvpce::Bounds& b, float d, int R, Cells* c) {
	const std::string many = dvpce::check_binned(b.finite);
	if (!many.empty()) return many;
	c->R = R;
	c->g.h = (double)d * (1.0 + 1.0 / 1024.0) / (double)R;
	for (int a = 0; a < 3; ++a) {
		c->g.origin[a] = b.finite ? (double)b.lo[a] - (double)(2 * R + 1) * c->g.h : 0.0;
		const double top = b.finite ? floor(((double)b.hi[a] - c->g.origin[a]) / c->g.h) : (double)(2 * R + 1);
		if (!(top + (double)(2 * R + 1) <= (double)dvpce::kMaxCellsPerAxis)) {
			char text[240];
			snprintf(text, sizeof text, "the targets extend over %.9g along axis %d, which is %.0f cells for the distance %.9g; at most %lld are supported",
			         (double)b.hi[a] - (double)b.lo[a], a, top + (double)(2 * R + 1), (double)d, dvpce::kMaxCellsPerAxis);
			return text;
		}
		c->t_max[a] = b.finite ? top + (double)R : -1.0;   // (no target: no source is searched)
	}
	return "";
}

// The 16 tree sums of leaves produced in index order: push(leaf) N times.
struct TreeSum {
	double part[64][16];
	int depth = 0;
	unsigned long long pushed = 0;
	void push(const double leaf[16]) {
		for (int k = 0; k < 16; ++k) part[depth][k] = leaf[k];
		++depth;
		for (unsigned long long t = ++pushed; !(t & 1ull); t >>= 1) {   // two finished subtrees of one size: their parent
			for (int k = 0; k < 16; ++k) part[depth - 2][k] = part[depth - 2][k] + part[depth - 1][k];
			--depth;
		}
	}
};

// One step on the host.  nearest (-1: none) and e_out (+inf: none) may be NULL.  `brute`: the double loop, else the grid walked
// serially.  "" or the error.
inline std::string serial_icp_step(const float* src, long long ns, const float* tgt, long long nt, const double* D, float d, int R, bool brute, int* nearest, float* e_out,
                                   double sums[16], long long* count) {
	std::string what = check_increment(D);
	if (what.empty()) what = check_distance(d);
	if (!what.empty()) return what;
	dvpce::Bounds b;
	b.add(tgt, nt);
	what = check_targets(b, nt);
	if (!what.empty()) return what;
	Cells cells;
	what = make_cells(b, d, R, &cells);
	if (!what.empty()) return what;
	const float d2max = d * d;
	double c[3];
	reference_point(b, c);
	dvpce::HostCells table;
	if (!brute) table.build(cells.g, tgt, nt, dvpce::table_capacity((uint64_t)nt));
	const int K = (2 * R + 1) * (2 * R + 1) * (2 * R + 1);
	TreeSum tree;
	const double zero[16] = { 0.0 };
	*count = 0;
	const long long N = padded(ns);
	for (long long i = 0; i < N; ++i) {
		if (i >= ns) { tree.push(zero); continue; }
		double p[3];
		float r[3], best = INFINITY;
		uint32_t best_j = kNoTarget;
		if (image_of(D, src[3 * i], src[3 * i + 1], src[3 * i + 2], p, r)) {
			if (brute) {
				for (long long j = 0; j < nt; ++j) {
					const float e = dvpce::sq_dist(r[0], r[1], r[2], tgt[3 * j], tgt[3 * j + 1], tgt[3 * j + 2]);
					if (closer(e, (uint32_t)j, best, best_j)) { best = e; best_j = (uint32_t)j; }
				}
			} else if (searched(cells, r[0], r[1], r[2])) {
				const uint64_t key = dvpce::cell_key(cells.g, r[0], r[1], r[2]);
				for (int n = 0; n < K; ++n) {
					const uint64_t s = table.find(neighbour_of(key, n, R));
					if (s == table.cap) continue;
					for (uint32_t at = table.start[s]; at < table.start[s + 1]; ++at) {
						const uint32_t j = table.index[at];
						const float e = dvpce::sq_dist(r[0], r[1], r[2], tgt[3 * (size_t)j], tgt[3 * (size_t)j + 1], tgt[3 * (size_t)j + 2]);
						if (closer(e, j, best, best_j)) { best = e; best_j = j; }
					}
				}
			}
		}
		const bool corresponds = best_j != kNoTarget && best <= d2max;
		if (nearest) nearest[i] = corresponds ? (int)best_j : -1;
		if (e_out) e_out[i] = corresponds ? best : INFINITY;
		if (!corresponds) { tree.push(zero); continue; }
		double leaf[16];
		leaf_of(p, tgt[3 * (size_t)best_j], tgt[3 * (size_t)best_j + 1], tgt[3 * (size_t)best_j + 2], c, best, leaf);
		tree.push(leaf);
		++*count;
	}
	for (int k = 0; k < 16; ++k) sums[k] = tree.part[0][k];
	return "";
}

// E (16 doubles) from the sums of n >= 3 correspondences about the reference point c
inline void solve(const double S[16], long long n, const double c[3], double E[16]) {
	const double dn = (double)n;
	double mua[3], mub[3], H[3][3];
	for (int r = 0; r < 3; ++r) { mua[r] = S[r] / dn; mub[r] = S[3 + r] / dn; }
	for (int r = 0; r < 3; ++r)
		for (int k = 0; k < 3; ++k) H[r][k] = S[6 + 3 * r + k] - (S[r] * S[3 + k]) / dn;
	double A[4][4] = {
		{ (H[0][0] + H[1][1]) + H[2][2], H[1][2] - H[2][1], H[2][0] - H[0][2], H[0][1] - H[1][0] },
		{ H[1][2] - H[2][1], (H[0][0] - H[1][1]) - H[2][2], H[0][1] + H[1][0], H[2][0] + H[0][2] },
		{ H[2][0] - H[0][2], H[0][1] + H[1][0], (-H[0][0] + H[1][1]) - H[2][2], H[1][2] + H[2][1] },
		{ H[0][1] - H[1][0], H[2][0] + H[0][2], H[1][2] + H[2][1], (-H[0][0] - H[1][1]) + H[2][2] } };
	double V[4][4] = { { 1, 0, 0, 0 }, { 0, 1, 0, 0 }, { 0, 0, 1, 0 }, { 0, 0, 0, 1 } };
	for (int sweep = 0; sweep < kSweepCap; ++sweep) {
		double off = 0.0, dia = 0.0;
		for (int p = 0; p < 4; ++p) {
			dia = dia + A[p][p] * A[p][p];
			for (int q = p + 1; q < 4; ++q) off = off + A[p][q] * A[p][q];
		}
		if (off <= 0x1p-106 * dia) break;
		for (int p = 0; p < 3; ++p)
			for (int q = p + 1; q < 4; ++q) {
				if (A[p][q] == 0.0) continue;
				const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
				const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
				const double co = 1.0 / sqrt(t * t + 1.0), si = t * co;
				for (int k = 0; k < 4; ++k) {
					const double akp = A[k][p], akq = A[k][q], vkp = V[k][p], vkq = V[k][q];
					A[k][p] = co * akp - si * akq;
					A[k][q] = si * akp + co * akq;
					V[k][p] = co * vkp - si * vkq;
					V[k][q] = si * vkp + co * vkq;
				}
				for (int k = 0; k < 4; ++k) {
					const double apk = A[p][k], aqk = A[q][k];
					A[p][k] = co * apk - si * aqk;
					A[q][k] = si * apk + co * aqk;
				}
			}
	}
	int top = 0;
	for (int p = 1; p < 4; ++p)
		if (A[p][p] > A[top][top]) top = p;
	double w = V[0][top], x = V[1][top], y = V[2][top], z = V[3][top];
	const double norm = sqrt(((w * w + x * x) + y * y) + z * z);
	w = w / norm; x = x / norm; y = y / norm; z = z / norm;
	const double R[3][3] = { { ((w * w + x * x) - y * y) - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y) },
		                     { 2.0 * (x * y + w * z), ((w * w - x * x) + y * y) - z * z, 2.0 * (y * z - w * x) },
		                     { 2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((w * w - x * x) - y * y) + z * z } };
	const double fa[3] = { mua[0] + c[0], mua[1] + c[1], mua[2] + c[2] };
	for (int r = 0; r < 3; ++r) {
		for (int k = 0; k < 3; ++k) E[4 * r + k] = R[r][k];
		E[4 * r + 3] = (mub[r] + c[r]) - ((R[r][0] * fa[0] + R[r][1] * fa[1]) + R[r][2] * fa[2]);
	}
	E[12] = E[13] = E[14] = 0.0;
	E[15] = 1.0;
}

// out = E * D (out may be neither)
inline void compose(const double* E, const double* D, double* out) {
	for (int r = 0; r < 3; ++r)
		for (int k = 0; k < 4; ++k) out[4 * r + k] = ((E[4 * r] * D[k] + E[4 * r + 1] * D[4 + k]) + E[4 * r + 2] * D[8 + k]) + E[4 * r + 3] * D[12 + k];
	out[12] = out[13] = out[14] = 0.0;
	out[15] = 1.0;
}

// The stages over a backend that prepares and steps:
//   std::string open_stage(const double M[16], double voxel, float d, long long* n_src, double c[3])
//   std::string step(const double D[16], double sums[16], long long* n)
//   void close_stage()
// M: the initial matrix in, the refined one out.  "" or the error.
template <class Backend>
std::string refine(Backend& be, const Stage* stages, int num_stages, double M[16], std::vector<LogRecord>* log) {
	std::string what = check_stages(stages, num_stages);
	if (!what.empty()) return what;
	for (int s = 0; s < num_stages; ++s) {
		long long n_src = 0;
		double c[3];
		what = be.open_stage(M, stages[s].voxel, (float)stages[s].max_distance, &n_src, c);
		double D[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
		double last_fitness = 0.0, last_rmse = 0.0;
		for (int step = 1; step <= stages[s].max_iterations && what.empty(); ++step) {
			double sums[16];
			long long n = 0;
			what = be.step(D, sums, &n);
			if (!what.empty()) break;
			const double fitness = n_src ? (double)n / (double)n_src : 0.0, rmse = n ? sqrt(sums[15] / (double)n) : 0.0;
			log->push_back(LogRecord{ s, step, n_src, n, rmse });
			if (n < 3) break;
			if (step >= 2 && fabs(fitness - last_fitness) < 1e-6 && fabs(rmse - last_rmse) < 1e-6) break;
			last_fitness = fitness;
			last_rmse = rmse;
			double E[16], next[16];
			solve(sums, n, c, E);
			compose(E, D, next);
			what = check_increment(next);
			for (int k = 0; k < 16; ++k) D[k] = next[k];
		}
		be.close_stage();
		if (!what.empty()) return "stage " + std::to_string(s) + ": " + what;
		double next[16];
		compose(D, M, next);
		for (int k = 0; k < 16; ++k) M[k] = next[k];
	}
	return "";
}

// the host flavour's backend: dvp_cloudprep.hpp's serial_prepare, serial_icp_step
struct HostBackend {
	const float* xyz[2];
	long long num[2];
	dvpcp::Prep prep[2];   // recon, truth: the crop of each (transform and voxel are the stage's)
	int R = 1;
	std::vector<float> src, tgt;
	float d = 0.0f;
	std::string open_stage(const double M[16], double voxel, float distance, long long* n_src, double c[3]) {
		d = distance;
		std::vector<float>* out[2] = { &src, &tgt };
		for (int k = 0; k < 2; ++k) {
			dvpcp::Prep p = prep[k];
			p.voxel = voxel;
			p.has_transform = k == 0;
			for (int e = 0; e < 16 && k == 0; ++e) p.m[e] = M[e];
			long long counts[4];
			const std::string what = dvpcp::serial_prepare(xyz[k], num[k], p, out[k], nullptr, counts);
			if (!what.empty()) return what;
		}
		dvpce::Bounds b;
		b.add(tgt.data(), (long long)(tgt.size() / 3));
		const std::string what = check_targets(b, (long long)(tgt.size() / 3));
		if (!what.empty()) return what;
		reference_point(b, c);
		*n_src = (long long)(src.size() / 3);
		return "";
	}
	std::string step(const double D[16], double sums[16], long long* n) {
		const long long ns = (long long)(src.size() / 3), nt = (long long)(tgt.size() / 3);
		return serial_icp_step(src.data(), ns, tgt.data(), nt, D, d, R, ns * nt <= dvpce::kBruteForcePairs, nullptr, nullptr, sums, n);
	}
	void close_stage() {}
};

// "" or what is wrong with a description handed to a refinement: the stage sets transform and voxel itself
inline std::string check_refine_prep(const dvpcp::Prep& p) {
	dvpcp::Prep q = p;
	q.voxel = 0.0;
	return dvpcp::check_prep(q);
}

// 1 (27 cells of edge d, the default: the faster one where measured, profiles/evaluate_refine.txt) or 2 (125 cells of edge d / 2)
// from DVP_CLOUD_ICP_CELLS = 27 | 125; 0: another value
inline int cells_radius_from_environment() {
	const char* v = getenv("DVP_CLOUD_ICP_CELLS");
	if (!v) return 1;
	const std::string s = v;
	return s == "27" ? 1 : s == "125" ? 2 : 0;
}

}   // namespace dvpci
#endif
