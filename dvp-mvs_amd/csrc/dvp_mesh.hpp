// dvp_mesh.hpp — the definition behind `dvp_mesh_*`: a truncated signed distance volume over a hashed grid of 8 x 8 x 8 blocks, filled
// from consistency-masked depth maps, and a surface-nets extraction of its zero level.  The project's own definition, pinned to no
// library.  The same text for the device (dvp_mesh.hip) and the test tool (tests/mesh_host); the SERIAL TEXT is the second half.
// Binary32 with one rounding per operator (-ffp-contract=off), binary64 only where said.
//   lattice    sample (i, j, k) sits at P = ((float)((double)i * s), ...), i, j, k in [-2^20, 2^20) ("21 bits, signed"); s the voxel edge
//   blocks     block (bx, by, bz) = (floor(i / 8), ...) holds 512 samples, local index l = lx * 64 + ly * 8 + lz; key = (bx + 2^20) << 42 |
//              (by + 2^20) << 21 | (bz + 2^20): 63 bits, ascending key = ascending (bx, by, bz), a forward neighbour's key never borrows
//   allocation the SET of the blocks of floor((double)X / (double)s) per axis, X = the lift of every masked pixel (mask != 0, depth
//              z > 0) at the depths z + (float)m * (s * 0.5f), m = -2M ... 2M, M = ceil((double)tau / (double)s), with the fusion's
//              pixel-to-world arithmetic (fuse_lift).  An index outside the lattice (a non-finite one too) refuses the build.
//   integration per sample, views in add_view order: project P with the fusion's world-to-pixel arithmetic (fuse_project), round
//              to the nearest pixel (fuse_round); skip unless depth zc > 0, the pixel is inside and masked, and sdf = d - zc >= -tau;
//              then SF += min(1, sdf / tau), W += 1, and where |sdf| <= tau the pixel's b, g, r are added to integer sums with a count.
//              F = SF / (float)W.
//   cells      cell (i, j, k) has the corners (i + dx, j + dy, k + dz), corner number c = dx * 4 + dy * 2 + dz; it belongs to the block
//              of its corner 0.  A corner is VALID when its block exists and W >= min_weight; it is inside when F < 0 (F >= 0, -0.0
//              included, is outside).  A cell is active iff all 8 corners are valid and not all on one side.
//   vertex     of an active cell: the mean of the crossings P0 + F0 / (F0 - F1) * (P1 - P0) over its sign-changing edges in the order
//              e = a * 4 + q (a the edge's axis; q = 2 u + v, (u, v) the offsets of the edge along the two other axes in x, y, z
//              order): the three coordinates are summed in that order and divided by (float)count.  Colour: the b, g, r sums and the
//              counts of the 8 corners added up, channel = (sum + n / 2) / n in integers, 0 when n == 0.
//   faces      sample o = (i, j, k) owns, per axis a, the lattice edge from o + (1, 1, 1) - e_a to o + (1, 1, 1): when its F values
//              change sign and the four cells o, o + e_b, o + e_b + e_c, o + e_c ((a, b, c) cyclic) are all active, their vertices
//              v0 v1 v2 v3 give the triangles (v0 v1 v2)(v0 v2 v3) when F rises along +a, else (v0 v2 v1)(v0 v3 v2): the normal
//              points to F >= 0.
//   order      blocks by ascending key, cells and owning samples by ascending local index, then axis: vertices and faces in that order.
#ifndef DVP_MESH_HPP_
#define DVP_MESH_HPP_

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/dvp_mvs.h"

#if defined(__HIPCC__)
#define DVP_MHD __host__ __device__ inline
#else
#define DVP_MHD inline
#endif

#include <algorithm>
#include <string>
#include <vector>

namespace dvpmesh {

constexpr int kBlockSamples = 512;
constexpr int kIndexLimit = 1 << 20;       // lattice indices are -2^20 ... 2^20 - 1
constexpr int kMaxBand = 64;               // M = ceil(tau / s) at most
constexpr uint64_t kEmptyKey = ~0ull;      // (no key has bit 63 set)
constexpr long long kMaxVertices = 2147483647ll;

struct View {
	DvpCamera cam;
	float centre[3];        // -R^T t in binary32, as the fusion has it
	int cols, rows;
	const float* depth;     // [rows * cols]
	const uint8_t* mask;    // [rows * cols]
	const uint8_t* bgr;     // [rows * cols * 3]
	float depth_max;        // the largest depth of a masked pixel, 0 without one (only the view cull reads it)
};

struct Params {
	float s, tau;
	int min_weight, M;
};

struct Sample {
	float sf;
	int w;
	uint32_t b, g, r, n;
};

DVP_MHD float lattice(int i, float s) { return (float)((double)i * (double)s); }
DVP_MHD int floor_div8(int i) { return (i >= 0 ? i : i - 7) / 8; }

DVP_MHD uint64_t block_key(int bx, int by, int bz) {
	return ((uint64_t)(bx + kIndexLimit) << 42) | ((uint64_t)(by + kIndexLimit) << 21) | (uint64_t)(bz + kIndexLimit);
}
DVP_MHD void key_block(uint64_t key, int b[3]) {
	b[0] = (int)(key >> 42) - kIndexLimit;
	b[1] = (int)((key >> 21) & 0x1fffffu) - kIndexLimit;
	b[2] = (int)(key & 0x1fffffu) - kIndexLimit;
}
// forward neighbour n = dx * 4 + dy * 2 + dz of a block
DVP_MHD uint64_t forward_key(uint64_t key, int n) {
	return key + ((uint64_t)(n >> 2) << 42) + ((uint64_t)((n >> 1) & 1) << 21) + (uint64_t)(n & 1);
}

// the home slot of a block is hash_key(key) & (capacity - 1)   (the finaliser of splitmix64, as the cloud evaluation's table has it)
DVP_MHD uint64_t hash_key(uint64_t k) {
	k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
	k ^= k >> 27; k *= 0x94d049bb133111ebull;
	k ^= k >> 31;
	return k;
}

DVP_MHD void set_centre(View* v) {
	for (int k = 0; k < 3; ++k) v->centre[k] = -(v->cam.R[0 + k] * v->cam.t[0] + v->cam.R[3 + k] * v->cam.t[1] + v->cam.R[6 + k] * v->cam.t[2]);
}

// pixel + depth -> world: fuse_lift's arithmetic
DVP_MHD void lift(const View& v, int x, int y, float z, float X[3]) {
	const float cx = z * (x - v.cam.K[2]) / v.cam.K[0];
	const float cy = z * (y - v.cam.K[5]) / v.cam.K[4];
	X[0] = (v.cam.R[0] * cx + v.cam.R[3] * cy + v.cam.R[6] * z) + v.centre[0];
	X[1] = (v.cam.R[1] * cx + v.cam.R[4] * cy + v.cam.R[7] * z) + v.centre[1];
	X[2] = (v.cam.R[2] * cx + v.cam.R[5] * cy + v.cam.R[8] * z) + v.centre[2];
}
// world -> pixel and depth: fuse_project's arithmetic
DVP_MHD void project(const float X[3], const DvpCamera& cam, float* px, float* py, float* depth) {
	const float tx = cam.R[0] * X[0] + cam.R[1] * X[1] + cam.R[2] * X[2] + cam.t[0];
	const float ty = cam.R[3] * X[0] + cam.R[4] * X[1] + cam.R[5] * X[2] + cam.t[1];
	const float tz = cam.R[6] * X[0] + cam.R[7] * X[1] + cam.R[8] * X[2] + cam.t[2];
	*depth = cam.K[6] * tx + cam.K[7] * ty + cam.K[8] * tz;
	*px = (cam.K[0] * tx + cam.K[1] * ty + cam.K[2] * tz) / *depth;
	*py = (cam.K[3] * tx + cam.K[4] * ty + cam.K[5] * tz) / *depth;
}
// fuse_round: int(v + 0.5f), a value no int holds lands outside every image
DVP_MHD int round_pixel(float v) {
	const float t = v + 0.5f;
	if (!(t > -2147483648.0f && t < 2147483648.0f)) return -1;
	return (int)t;
}

DVP_MHD bool masked(const View& v, size_t p) { return v.mask[p] != 0 && v.depth[p] > 0.0f; }

// the block of step m of a masked pixel's band; false: a lattice index beyond 21 bits
DVP_MHD bool band_key(const View& v, const Params& p, int x, int y, float z, int m, uint64_t* key) {
	const float zm = z + (float)m * (p.s * 0.5f);
	float X[3];
	lift(v, x, y, zm, X);
	int b[3];
	for (int a = 0; a < 3; ++a) {
		const double q = floor((double)X[a] / (double)p.s);
		if (!(q >= -(double)kIndexLimit && q < (double)kIndexLimit)) return false;
		b[a] = floor_div8((int)q);
	}
	*key = block_key(b[0], b[1], b[2]);
	return true;
}

// one view's share of the sample at P
DVP_MHD void integrate(const View& v, float tau, const float P[3], Sample* a) {
	float px, py, zc;
	project(P, v.cam, &px, &py, &zc);
	if (!(zc > 0.0f)) return;
	const int x = round_pixel(px), y = round_pixel(py);
	if (x < 0 || x >= v.cols || y < 0 || y >= v.rows) return;
	const size_t p = (size_t)y * v.cols + x;
	if (!masked(v, p)) return;
	const float sdf = v.depth[p] - zc;
	if (!(sdf >= -tau)) return;
	const float r = sdf / tau;
	a->sf = a->sf + (r < 1.0f ? r : 1.0f);
	a->w += 1;
	if (fabsf(sdf) <= tau) {
		a->b += v.bgr[3 * p];
		a->g += v.bgr[3 * p + 1];
		a->r += v.bgr[3 * p + 2];
		a->n += 1;
	}
}

// ---- the view cull: which views a whole block may skip.  Not part of the definition (the serial text integrates every view); the device
// calls these three and tests/mesh_host's `cull` mode runs the same text, so that its soundness is a host test.

// the sphere around the samples of block `at`: they lie within half the diagonal of a 7 s cube of its centre
DVP_MHD void block_sphere(const int at[3], float s, float C[3], float* radius) {
	for (int a = 0; a < 3; ++a) C[a] = (float)(((double)at[a] * 8.0 + 3.5) * (double)s);
	*radius = s * 6.0622f + fabsf(C[0]) * 1e-6f + fabsf(C[1]) * 1e-6f + fabsf(C[2]) * 1e-6f;   // 3.5 sqrt(3) = 6.06218
}

DVP_MHD bool orthonormal(const float* R) {
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			const double d = (double)R[3 * i] * R[3 * j] + (double)R[3 * i + 1] * R[3 * j + 1] + (double)R[3 * i + 2] * R[3 * j + 2];
			if (!(fabs(d - (i == j ? 1.0 : 0.0)) < 1e-4)) return false;
		}
	return true;
}

// the camera has K's last row 0 0 1, no skew and an orthonormal R: the sphere test of view_misses_block is valid
DVP_MHD bool cullable(const DvpCamera& cam) {
	const float* K = cam.K;
	return K[6] == 0.0f && K[7] == 0.0f && K[8] == 1.0f && K[1] == 0.0f && K[3] == 0.0f && K[0] > 0.0f && K[4] > 0.0f && orthonormal(cam.R);
}

// true only when no sample within `radius` of C (world) can see a masked pixel of the view with sdf >= -tau.  Every bound carries
// a margin far above the rounding of the per-sample arithmetic (half a pixel and more, a quarter of the radius, 1e-3 of the distance).
DVP_MHD bool view_misses_block(const View& v, bool cullable, const float C[3], float radius, float tau) {
	if (!(v.depth_max > 0.0f)) return true;   // no masked pixel at all
	if (!cullable) return false;
	const float* R = v.cam.R;
	const float tx = R[0] * C[0] + R[1] * C[1] + R[2] * C[2] + v.cam.t[0];
	const float ty = R[3] * C[0] + R[4] * C[1] + R[5] * C[2] + v.cam.t[1];
	const float tz = R[6] * C[0] + R[7] * C[1] + R[8] * C[2] + v.cam.t[2];
	const float r = radius * 1.25f + 1e-3f * (sqrtf(tx * tx + ty * ty + tz * tz) + radius);
	if (!(r == r) || !(tz == tz)) return false;
	if (tz + r <= 0.0f) return true;
	if (tz - r > v.depth_max + tau) return true;
	const float fx = v.cam.K[0], fy = v.cam.K[4], cx = v.cam.K[2], cy = v.cam.K[5];
	// a visible sample q (camera frame, q.z > 0) has -1.5 < px < cols - 0.5 (int(px + 0.5f) truncates towards zero), py likewise:
	// four half-spaces through the centre, at -2 and cols + 1
	const float nx0 = cx + 2.0f, nx1 = (float)v.cols + 1.0f - cx, ny0 = cy + 2.0f, ny1 = (float)v.rows + 1.0f - cy;
	if (fx * tx + nx0 * tz < -r * sqrtf(fx * fx + nx0 * nx0)) return true;
	if (-fx * tx + nx1 * tz < -r * sqrtf(fx * fx + nx1 * nx1)) return true;
	if (fy * ty + ny0 * tz < -r * sqrtf(fy * fy + ny0 * ny0)) return true;
	if (-fy * ty + ny1 * tz < -r * sqrtf(fy * fy + ny1 * ny1)) return true;
	return false;
}

// F of a valid sample, NaN of one that is not
DVP_MHD float sample_f(float sf, int w, int min_weight) { return w >= min_weight ? sf / (float)w : NAN; }

DVP_MHD bool cell_active(const float F[8]) {
	int inside = 0;
	for (int c = 0; c < 8; ++c) {
		if (F[c] != F[c]) return false;
		inside += F[c] < 0.0f;
	}
	return inside > 0 && inside < 8;
}

// the vertex of the active cell (i, j, k)
DVP_MHD void cell_vertex(const float F[8], int i, int j, int k, float s, float out[3]) {
	const int at[3] = { i, j, k };
	float sum[3] = { 0.0f, 0.0f, 0.0f };
	int count = 0;
	for (int a = 0; a < 3; ++a) {
		const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;   // the two other axes in x, y, z order
		for (int q = 0; q < 4; ++q) {
			int d[3];
			d[a] = 0; d[b] = q >> 1; d[c] = q & 1;
			const int c0 = d[0] * 4 + d[1] * 2 + d[2], c1 = c0 + (4 >> a);
			const float F0 = F[c0], F1 = F[c1];
			if ((F0 < 0.0f) == (F1 < 0.0f)) continue;
			float X[3];
			for (int e = 0; e < 3; ++e) X[e] = lattice(at[e] + d[e], s);
			const float P1 = lattice(at[a] + 1, s);
			X[a] = X[a] + F0 / (F0 - F1) * (P1 - X[a]);
			for (int e = 0; e < 3; ++e) sum[e] = sum[e] + X[e];
			++count;
		}
	}
	for (int e = 0; e < 3; ++e) out[e] = sum[e] / (float)count;
}

DVP_MHD uint8_t mean_colour(uint32_t sum, uint32_t n) { return n ? (uint8_t)((sum + n / 2) / n) : (uint8_t)0; }

// the lattice edge from F0 to F1 along +a: 0 no face, 1 F rises (normal along +a), 2 F falls
DVP_MHD int edge_face(float F0, float F1) {
	if (F0 != F0 || F1 != F1 || (F0 < 0.0f) == (F1 < 0.0f)) return 0;
	return F0 < 0.0f ? 1 : 2;
}
// the local offsets of the four cells around sample o's edge of axis a, in quad order
DVP_MHD void quad_cell(int a, int q, int d[3]) {
	const int b = (a + 1) % 3, c = (a + 2) % 3;
	d[a] = 0;
	d[b] = q == 1 || q == 2;
	d[c] = q == 2 || q == 3;
}
// the six indices of a quad's two triangles
DVP_MHD void quad_faces(int kind, const int v[4], int* out) {
	if (kind == 1) { out[0] = v[0]; out[1] = v[1]; out[2] = v[2]; out[3] = v[0]; out[4] = v[2]; out[5] = v[3]; }
	else           { out[0] = v[0]; out[1] = v[2]; out[2] = v[1]; out[3] = v[0]; out[4] = v[3]; out[5] = v[2]; }
}

// ---- host part: argument checks and the serial text ------------------------------------------------------------------------------

// "" or what is wrong; fills *p
inline std::string check_params(float s, float tau, int min_weight, Params* p) {
	char text[200];
	if (!(s > 0.0f) || !((s - s) == 0.0f)) {
		snprintf(text, sizeof text, "the voxel edge must be finite and positive, got %.9g", (double)s);
		return text;
	}
	if (!((tau - tau) == 0.0f) || !(tau >= s)) {
		snprintf(text, sizeof text, "the truncation distance (%.9g) must be finite and at least the voxel edge (%.9g)", (double)tau, (double)s);
		return text;
	}
	const double M = ceil((double)tau / (double)s);
	if (!(M <= (double)kMaxBand)) {
		snprintf(text, sizeof text, "the truncation distance (%.9g) spans more than %d voxels of %.9g", (double)tau, kMaxBand, (double)s);
		return text;
	}
	if (min_weight < 1) return "min_weight must be at least 1, got " + std::to_string(min_weight);
	p->s = s; p->tau = tau; p->min_weight = min_weight; p->M = (int)M;
	return "";
}
inline std::string check_view(int cols, int rows) {
	if (cols < 1 || rows < 1 || (long long)cols * rows > 2147483647ll) return "a view has 1 ... 2^31 - 1 pixels, got " + std::to_string(cols) + " x " + std::to_string(rows);
	return "";
}
inline std::string index_refusal(int view) {
	return "a lattice index beyond 21 bits (view " + std::to_string(view) + "): the scene spans more than 2^21 voxels, or a masked depth is not finite";
}
inline std::string vertex_refusal(long long vertices) {
	return "the mesh has " + std::to_string(vertices) + " vertices; an int face index holds at most " + std::to_string(kMaxVertices);
}

inline float masked_depth_max(const View& v) {
	float m = 0.0f;
	for (size_t p = 0, L = (size_t)v.cols * v.rows; p < L; ++p)
		if (masked(v, p) && v.depth[p] > m) m = v.depth[p];
	return m;
}

struct Volume {
	std::vector<uint64_t> keys;       // ascending
	std::vector<float> sf;            // [blocks * 512]
	std::vector<int> w;
	std::vector<uint32_t> colour;     // [blocks * 512 * 4]: b, g, r sums and the count
	std::vector<int> forward;         // [blocks * 8]: the block of forward neighbour n (0 = itself), -1 = none
};
struct Mesh {
	std::vector<float> vertices;      // x y z
	std::vector<uint8_t> colours;     // b g r
	std::vector<int> faces;           // three indices
};

// the set of allocated blocks, ascending; "" or the refusal
inline std::string serial_blocks(const std::vector<View>& views, const Params& p, std::vector<uint64_t>* keys) {
	keys->clear();
	auto tidy = [keys]() {
		std::sort(keys->begin(), keys->end());
		keys->erase(std::unique(keys->begin(), keys->end()), keys->end());
	};
	size_t tidied = 0;
	for (size_t n = 0; n < views.size(); ++n) {
		const View& v = views[n];
		for (int y = 0; y < v.rows; ++y)
			for (int x = 0; x < v.cols; ++x) {
				const size_t at = (size_t)y * v.cols + x;
				if (!masked(v, at)) continue;
				for (int m = -2 * p.M; m <= 2 * p.M; ++m) {
					uint64_t key;
					if (!band_key(v, p, x, y, v.depth[at], m, &key)) return index_refusal((int)n);
					if (keys->empty() || keys->back() != key) keys->push_back(key);
				}
				if (keys->size() > tidied + (1u << 22)) { tidy(); tidied = keys->size(); }
			}
	}
	tidy();
	return "";
}

inline int find_block(const std::vector<uint64_t>& keys, uint64_t key) {
	const auto it = std::lower_bound(keys.begin(), keys.end(), key);
	return it != keys.end() && *it == key ? (int)(it - keys.begin()) : -1;
}

// SF, W and the colour sums of every sample of the blocks vol->keys, and the forward neighbours
inline void serial_integrate(const std::vector<View>& views, const Params& p, Volume* vol) {
	const size_t blocks = vol->keys.size();
	vol->sf.assign(blocks * kBlockSamples, 0.0f);
	vol->w.assign(blocks * kBlockSamples, 0);
	vol->colour.assign(blocks * kBlockSamples * 4, 0u);
	vol->forward.assign(blocks * 8, -1);
	for (size_t b = 0; b < blocks; ++b) {
		for (int n = 0; n < 8; ++n) vol->forward[b * 8 + n] = find_block(vol->keys, forward_key(vol->keys[b], n));
		int at[3];
		key_block(vol->keys[b], at);
		for (int l = 0; l < kBlockSamples; ++l) {
			const float P[3] = { lattice(at[0] * 8 + (l >> 6), p.s), lattice(at[1] * 8 + ((l >> 3) & 7), p.s), lattice(at[2] * 8 + (l & 7), p.s) };
			Sample a = { 0.0f, 0, 0u, 0u, 0u, 0u };
			for (const View& v : views) integrate(v, p.tau, P, &a);
			const size_t i = b * kBlockSamples + l;
			vol->sf[i] = a.sf;
			vol->w[i] = a.w;
			vol->colour[4 * i] = a.b; vol->colour[4 * i + 1] = a.g; vol->colour[4 * i + 2] = a.r; vol->colour[4 * i + 3] = a.n;
		}
	}
}

// the sample at local (lx, ly, lz), each 0 ... 15, seen from block b: its index in the volume's arrays, or -1
inline long long sample_at(const Volume& vol, size_t b, int lx, int ly, int lz) {
	const int nb = vol.forward[b * 8 + (lx >> 3) * 4 + (ly >> 3) * 2 + (lz >> 3)];
	return nb < 0 ? -1 : (long long)nb * kBlockSamples + (lx & 7) * 64 + (ly & 7) * 8 + (lz & 7);
}

// "" or the refusal
inline std::string serial_extract(const Params& p, const Volume& vol, Mesh* mesh) {
	const size_t blocks = vol.keys.size();
	mesh->vertices.clear(); mesh->colours.clear(); mesh->faces.clear();
	std::vector<int> cell_vertex_of(blocks * kBlockSamples, -1);
	long long vertices = 0;
	for (size_t b = 0; b < blocks; ++b) {
		int at[3];
		key_block(vol.keys[b], at);
		for (int l = 0; l < kBlockSamples; ++l) {
			const int lx = l >> 6, ly = (l >> 3) & 7, lz = l & 7;
			float F[8];
			uint32_t sum[4] = { 0u, 0u, 0u, 0u };
			for (int c = 0; c < 8; ++c) {
				const long long i = sample_at(vol, b, lx + (c >> 2), ly + ((c >> 1) & 1), lz + (c & 1));
				F[c] = i < 0 ? NAN : sample_f(vol.sf[(size_t)i], vol.w[(size_t)i], p.min_weight);
				for (int e = 0; e < 4 && i >= 0; ++e) sum[e] += vol.colour[4 * (size_t)i + e];
			}
			if (!cell_active(F)) continue;
			if (vertices == kMaxVertices) return vertex_refusal(vertices + 1);
			cell_vertex_of[b * kBlockSamples + l] = (int)vertices++;
			float X[3];
			cell_vertex(F, at[0] * 8 + lx, at[1] * 8 + ly, at[2] * 8 + lz, p.s, X);
			for (int e = 0; e < 3; ++e) {
				mesh->vertices.push_back(X[e]);
				mesh->colours.push_back(mean_colour(sum[e], sum[3]));
			}
		}
	}
	for (size_t b = 0; b < blocks; ++b)
		for (int l = 0; l < kBlockSamples; ++l) {
			const int o[3] = { l >> 6, (l >> 3) & 7, l & 7 };
			for (int a = 0; a < 3; ++a) {
				int e0[3] = { o[0] + 1, o[1] + 1, o[2] + 1 };
				const long long i1 = sample_at(vol, b, e0[0], e0[1], e0[2]);
				e0[a] -= 1;
				const long long i0 = sample_at(vol, b, e0[0], e0[1], e0[2]);
				if (i0 < 0 || i1 < 0) continue;
				const int kind = edge_face(sample_f(vol.sf[(size_t)i0], vol.w[(size_t)i0], p.min_weight), sample_f(vol.sf[(size_t)i1], vol.w[(size_t)i1], p.min_weight));
				if (!kind) continue;
				int v[4];
				bool all = true;
				for (int q = 0; q < 4 && all; ++q) {
					int d[3];
					quad_cell(a, q, d);
					const long long i = sample_at(vol, b, o[0] + d[0], o[1] + d[1], o[2] + d[2]);
					v[q] = i < 0 ? -1 : cell_vertex_of[(size_t)i];
					all = v[q] >= 0;
				}
				if (!all) continue;
				int six[6];
				quad_faces(kind, v, six);
				mesh->faces.insert(mesh->faces.end(), six, six + 6);
			}
		}
	return "";
}

// the whole build; "" or the refusal
inline std::string serial_build(const std::vector<View>& views, const Params& p, Volume* vol, Mesh* mesh) {
	const std::string what = serial_blocks(views, p, &vol->keys);
	if (!what.empty()) return what;
	serial_integrate(views, p, vol);
	return serial_extract(p, *vol, mesh);
}

}   // namespace dvpmesh
#endif
